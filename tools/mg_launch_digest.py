#!/usr/bin/env python3
"""Launch digest of the multigrid PCG in its five modes, to compare two builds of the library (NOTES §R30.1).

  mg_launch_digest.py --list                   the 14 case names
  mg_launch_digest.py run CASE OUT.json        one call with the library CCP_GS_LIB names; sha256 of x per channel and the
                                               reports' bytes go to OUT.json.  Run it under `rocprofv3 --kernel-trace
                                               --output-format csv -d ROOT/trace/CASE/{parent,new} -o t --`, in a fresh
                                               process per case and library, with OUT = ROOT/res/CASE.{parent,new}.json
  mg_launch_digest.py compare ROOT OUT.jsonl   per case: the ordered dispatches (kernel name, grid, workgroup, LDS bytes) and
                                               the result bytes of the two libraries

Cases: weighted 70x40, C = 3, rescaled, screened weights (floating ones in the constant mode); ccp_grid_mg_conjugate_gradient
with cap 17 and epsilon 0, and ccp_grid_mg_apply, in the modes f64 (sequential, point), f32, batched, line and constant; and,
in the modes f64 and f32, `refresh` (ccp_grid_mg_prepare, ccp_grid_refresh_weights_device with other weights, then the same
synchronous solve) and `enqueue` (ccp_grid_mg_prepare, then ccp_grid_mg_conjugate_gradient_enqueue with cap 17).  These two
need torch for their device tensors."""
import csv, glob, hashlib, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

MODES = {"f64": {}, "f32": {"precision": "f32"}, "batched": {"channels": "batched"}, "line": {"smoother": "line"},
         "constant": {"nullspace": "constant"}}


def cases():
    return [f"{m}_{op}" for m in MODES for op in ("pcg", "apply")] + [f"{m}_{op}" for m in ("f64", "f32") for op in ("refresh", "enqueue")]


def run(name, out_path):
    from coursecomputationalphotography_amd import capi
    mode, op = name.rsplit("_", 1)
    W, H, C = 70, 40, 3
    rng = np.random.default_rng(7)
    wx, wy = (rng.uniform(0.5, 2.0, (H, W)).astype(np.float32) for _ in range(2))
    lam = None if mode == "constant" else np.full((H, W), 1e-2, dtype=np.float32)
    g = capi.Grid(W, H, C, weighted=True)
    g.mg_set_hierarchy("rescaled")
    for option, value in MODES[mode].items():
        getattr(g, f"mg_set_{option}")(value)
    g.set_weights(wx, wy, lam)
    g.randomize_x(1234, 0.0, 255.0)
    g.b_from_x()
    g.randomize_x(1235, 0.0, 255.0)
    if op in ("refresh", "enqueue"):
        import torch
        g.mg_prepare(0)
    if op == "refresh":
        w2 = [torch.from_numpy(rng.uniform(0.5, 2.0, (H, W))).cuda() for _ in range(2)]
        g.refresh_weights_tensor(w2[0], w2[1], torch.full((H, W), 1e-2, dtype=torch.float64, device="cuda"))
    if op == "enqueue":
        report = torch.zeros(C, 6, dtype=torch.float64, device="cuda")
        g.mg_conjugate_gradient_enqueue(0.0, 17, 0, report)
        torch.cuda.synchronize()
        reps = None
        enqueue_report = report.cpu().numpy()[:, :3]
    else:
        reps = g.mg_conjugate_gradient(0.0, 17, 0) if op in ("pcg", "refresh") else g.mg_apply(0)
    xs = [g.get_x(c) for c in range(C)]
    rep = np.array([[r.iterations, r.converged, r.last_l1_step] for r in reps or []], dtype=np.float64)
    if op == "enqueue":
        rep = np.ascontiguousarray(enqueue_report, dtype=np.float64)
    g.close()
    with open(out_path, "w") as f:
        json.dump({"case": name, "lib": os.environ.get("CCP_GS_LIB", "default"), "x_sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in xs],
                   "x_finite": bool(all(np.isfinite(x).all() for x in xs)), "report_hex": rep.tobytes().hex(), "reports": rep.tolist()}, f)
    print("done", name, rep.tolist(), flush=True)


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
    return [(col(r, "Kernel_Name"), tuple(int(col(r, f"Grid_Size_{a}")) for a in "XYZ"), tuple(int(col(r, f"Workgroup_Size_{a}")) for a in "XYZ"),
             int(col(r, "LDS_Block_Size", "LDS_Block_Size_Bytes"))) for r in rows]


def compare(root, out_path):
    all_ok = True
    with open(out_path, "w") as out:
        for c in cases():
            p, n = dispatches(os.path.join(root, "trace", c, "parent")), dispatches(os.path.join(root, "trace", c, "new"))
            rp, rn = (json.load(open(os.path.join(root, "res", f"{c}.{s}.json"))) for s in ("parent", "new"))
            digest = lambda l: hashlib.sha256(json.dumps(l).encode()).hexdigest()[:16]
            rec = {"case": c, "dispatches_parent": len(p), "dispatches_new": len(n), "hash_parent": digest(p), "hash_new": digest(n),
                   "same_dispatches": p == n, "x_bytes_equal": rp["x_sha256"] == rn["x_sha256"], "report_bytes_equal": rp["report_hex"] == rn["report_hex"],
                   "x_finite": rn["x_finite"], "reports": rn["reports"]}
            if p != n:
                rec["first_differences"] = [[i, str(a), str(b)] for i, (a, b) in enumerate(zip(p, n)) if a != b][:4]
            ok = rec["same_dispatches"] and rec["x_bytes_equal"] and rec["report_bytes_equal"] and rec["x_finite"]
            all_ok &= ok
            out.write(json.dumps(rec) + "\n")
            print("OK  " if ok else "FAIL", c, len(p), len(n), rec["reports"])
    print("ALL OK" if all_ok else "SOME FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(cases()))
    elif sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
