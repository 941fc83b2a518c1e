#!/usr/bin/env python3
"""Launch digest of the grid solve entry points, to compare two builds of the library (NOTES §R22.1).

  grid_launch_digest.py --list                 the 27 case names
  grid_launch_digest.py run CASE OUT.json      one small solve with the library CCP_GS_LIB names; sha256 of x per channel and
                                               the reports' bytes go to OUT.json.  Run it under `rocprofv3 --kernel-trace
                                               --output-format csv -d ROOT/trace/CASE/{parent,new} -o t --`, in a fresh
                                               process per case and library, with OUT = ROOT/res/CASE.{parent,new}.json
  grid_launch_digest.py compare ROOT           per case: the ordered dispatches (kernel name, grid, workgroup, LDS bytes) and
                                               the result bytes of the two libraries; writes ROOT/launch_digest.jsonl

Cases: 96x80, C = 2 (the system of test_world1_full_rccl_path) and a Dirichlet-mask grid 160x120: Gauss-Seidel on one block
and on a one-rank row block over real RCCL, fused passes on and off; CG in its three loops; the lexicographic solve."""
import csv, glob, hashlib, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np

GS_ARGS = {"e05_600_1": (0.5, 600, 1), "e05_600_3": (0.5, 600, 3), "e0_13_1": (0.0, 13, 1), "e0_33_0": (0.0, 33, 0)}


def cases():
    out = []
    for a in GS_ARGS:
        for f in ("fused", "unfused"):
            out.append(f"gs1_{f}_{a}")
            out.append(f"gsrb_{f}_{a}")
    out += ["gs1_mask", "gsrb_mask"]
    out += ["cg1_unset", "cg1_2", "cg1_0", "cgrb_unset", "cgrb_0", "cg1_mask", "cgrb_mask"]
    out += ["lex_checked", "lex_fixed"]
    return out


def run(name, out_path):
    kind, _, rest = name.partition("_")
    env = {}
    if kind == "gsrb" and rest.startswith("unfused"):
        env["CCP_GS_ROWBLOCK_CHECKED_FUSED"] = "0"
    if kind in ("cg1", "cgrb") and rest in ("2", "0"):
        env["CCP_GS_CG_FUSED"] = rest
    os.environ.pop("CCP_GS_CG_FUSED", None)
    os.environ.pop("CCP_GS_ROWBLOCK_CHECKED_FUSED", None)
    os.environ.update(env)
    from coursecomputationalphotography_amd import capi, synth
    masked = rest == "mask"
    W, H, C = (160, 120, 2) if masked else (96, 80, 2)
    mask = synth.disc_mask(W, H, seed=4321, n_discs=12, rmin=300.0, rmax=1400.0).astype(np.uint8) if masked else None
    base = synth.poisson_system(W, H, 1234)[0].reshape(H, W)
    g = capi.Grid(W, H, C, mask=mask) if masked else capi.Grid(W, H, C)
    g.set_b(base * 1e-3, 0)
    g.set_b(base * 3e-4, 1)
    comm = None
    if kind.endswith("rb"):
        comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
        g.attach_comm(comm)
    if kind in ("gs1", "gsrb"):
        g.fill_x(1.0)
        if masked:
            args = (5.0, 600, 1)
        else:
            f, _, a = rest.partition("_")
            args = GS_ARGS[a]
            if kind == "gs1" and f == "unfused":
                g.set_fused(False)
        reps = g.gauss_seidel(*args) if kind == "gs1" else g.gauss_seidel_rowblocked(*args)
    elif kind in ("cg1", "cgrb"):
        g.fill_x(0.0)
        reps = g.conjugate_gradient(1e-30, 20) if kind == "cg1" else g.conjugate_gradient_rowblocked(1e-30, 20)
    else:
        g.fill_x(1.0)
        reps = g.gauss_seidel_lexicographic(0.5, 600, 1) if rest == "checked" else g.gauss_seidel_lexicographic(0.0, 33, 0)
    xs = [g.get_x(ch) for ch in range(C)]
    rep = np.array([[r.iterations, r.converged, r.last_l1_step] for r in reps], dtype=np.float64)
    res = {"case": name, "lib": os.environ.get("CCP_GS_LIB", "default"), "env": env,
           "x_sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in xs], "x_finite": bool(all(np.isfinite(x).all() for x in xs)),
           "report_hex": rep.tobytes().hex(), "reports": rep.tolist()}
    if comm is not None:
        g.attach_comm(None)
    g.close()
    if comm is not None:
        comm.close()
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("done", name, res["reports"], flush=True)




def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError((names, list(row)))


def dispatches(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(col(r, "Dispatch_Id")))
    return [(col(r, "Kernel_Name"),
             tuple(int(col(r, f"Grid_Size_{a}")) for a in "XYZ"),
             tuple(int(col(r, f"Workgroup_Size_{a}")) for a in "XYZ"),
             int(col(r, "LDS_Block_Size", "LDS_Block_Size_Bytes"))) for r in rows]


def digest(lst):
    return hashlib.sha256(json.dumps(lst).encode()).hexdigest()[:16]


def compare(root):
    all_ok = True
    with open(os.path.join(root, "launch_digest.jsonl"), "w") as out:
        for c in cases():
            p, n = dispatches(os.path.join(root, "trace", c, "parent")), dispatches(os.path.join(root, "trace", c, "new"))
            rp, rn = (json.load(open(os.path.join(root, "res", f"{c}.{s}.json"))) for s in ("parent", "new"))
            diffs = [(i, a, b) for i, (a, b) in enumerate(zip(p, n)) if a != b]
            # the one expected difference: k_decide_sums' workgroup (64 -> kMaxChannels) on row blocks
            other = [d for d in diffs if not ("k_decide_sums" in d[1][0] and d[1][0] == d[2][0] and d[1][1] != d[2][1] and d[1][3] == d[2][3]
                                              and d[1][1][0] // d[1][2][0] == d[2][1][0] // d[2][2][0])]
            # the runtime's own copy kernels (hipMemcpyAsync / hipMemsetAsync, the read-back of x by the case script among them)
            ours = lambda l: [x for x in l if not x[0].startswith("__amd_rocclr_")]
            pdiffs = [(a, b) for a, b in zip(ours(p), ours(n)) if a != b and "k_decide_sums" not in a[0]]
            rec = {"case": c, "env": rn["env"], "dispatches_parent": len(p), "dispatches_new": len(n), "hash_parent": digest(p), "hash_new": digest(n),
                   "same_dispatches": len(p) == len(n) and not diffs,
                   "same_but_decide_sums_workgroup": len(p) == len(n) and not other, "decide_sums_workgroup_diffs": len(diffs) - len(other),
                   "decide_sums_workgroup": sorted({(d[1][2][0], d[2][2][0]) for d in diffs if d not in other}),
                   "dispatches_without_runtime_copies": [len(ours(p)), len(ours(n))],
                   "same_without_runtime_copies_but_decide_sums_workgroup": len(ours(p)) == len(ours(n)) and not pdiffs,
                   "x_bytes_equal": rp["x_sha256"] == rn["x_sha256"], "report_bytes_equal": rp["report_hex"] == rn["report_hex"],
                   "x_finite": rn["x_finite"], "reports": rn["reports"]}
            if other or len(p) != len(n):
                rec["first_differences"] = [list(map(str, d)) for d in other[:4]]
            ok = rec["same_without_runtime_copies_but_decide_sums_workgroup"] and rec["x_bytes_equal"] and rec["report_bytes_equal"]
            all_ok &= ok
            out.write(json.dumps(rec) + "\n")
            print("OK  " if ok and rec["same_but_decide_sums_workgroup"] else "ok* " if ok else "FAIL", c, rec["dispatches_parent"], rec["dispatches_new"], "decide wg diffs", rec["decide_sums_workgroup_diffs"], rec["reports"])
    print("ALL OK" if all_ok else "SOME FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(cases()))
    elif sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2]))
