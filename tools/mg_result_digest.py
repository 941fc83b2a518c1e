#!/usr/bin/env python3
"""Result digest of the multigrid PCG and of the CG passes, to compare two builds of the library bit for bit (NOTES §R25.1).

  mg_result_digest.py --list                      the case names
  mg_result_digest.py run OUT.json                every case with the library CCP_GS_LIB names, in a fresh process per
                                                  library; sha256 of every channel's x bytes and the reports go to OUT.json
  mg_result_digest.py compare A.json B.json OUT   per case whether the hashes and the reports are equal; writes OUT (jsonl)

Main cases: the handles and systems of tests/test_gpu_mg_batched.py (kinds structured, mask, galerkin, rescaled,
rescaled_fixed) at 5x3, 63x33, 64x64, 70x40 and 257x131 with C = 3, nu = 1 and 2, ccp_grid_mg_apply and
ccp_grid_mg_conjugate_gradient (1e-10 |b|, cap 40), in the modes fp64 sequential, fp64 batched and fp32.  Further cases: a
one-rank row block over real RCCL at 96x80 (k_mg_tile / k_mg_restrict with lo / hi), ccp_grid_conjugate_gradient on one
block in the fused and the three-pass loop, and CsrMatrix.conjugate_gradient on a stored matrix (the k_cg_* passes outside
multigrid)."""
import hashlib, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

KINDS = ["structured", "mask", "galerkin", "rescaled", "rescaled_fixed"]
SHAPES = [(5, 3), (63, 33), (64, 64), (70, 40), (257, 131)]
MODES = {"f64_sequential": ("f64", "sequential"), "f64_batched": ("f64", "batched"), "f32": ("f32", "sequential")}
EXTRA = ["rowblock_96x80", "grid_cg_fused", "grid_cg_three_pass", "csr_cg_stored"]


def cases():
    return [f"{kind}_{W}x{H}_{mode}_nu{nu}_{op}" for kind in KINDS for W, H in SHAPES for mode in MODES for nu in (1, 2)
            for op in ("apply", "pcg")] + EXTRA


def record(out, name, xs, reps=None):
    rep = np.array([[r.iterations, r.converged, r.last_l1_step] for r in reps or []], dtype=np.float64)
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    out[name] = {"x_sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in xs], "x_finite": bool(all(np.isfinite(x).all() for x in xs)),
                 "report_hex": rep.tobytes().hex(), "reports": rep.tolist()}


def run(out_path):
    import test_gpu_mg_batched as tb                        # its handle() and system() are the definition of the main cases
    from coursecomputationalphotography_amd import capi, synth
    out, Cn = {}, 3
    for kind in KINDS:
        for W, H in SHAPES:
            g = tb.handle(kind, W, H, Cn)
            bs, x0s = tb.system(g, 100 + W + Cn)
            eps = 1e-10 * float(np.linalg.norm(bs[0]))
            for mode, (precision, channels) in MODES.items():
                g.mg_set_precision(precision)
                g.mg_set_channels(channels)
                for nu in (1, 2):
                    for op in ("apply", "pcg"):
                        for c, x in enumerate(x0s):
                            g.set_x(x, c)
                        reps = g.mg_apply(nu) if op == "apply" else g.mg_conjugate_gradient(eps, 40, nu)
                        record(out, f"{kind}_{W}x{H}_{mode}_nu{nu}_{op}", [g.get_x(c) for c in range(Cn)], reps)
            g.close()
    # a one-rank row block: the levels carry lo / hi and ghost rows
    W, H, Cn = 96, 80, 2
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
    g = capi.Grid(W, H, Cn, 0, H, 1, 0)
    g.randomize_x(1234, 0.0, 255.0)
    g.b_from_x()
    g.randomize_x(1235, 0.0, 255.0)
    g.attach_comm(comm)
    g.mg_apply_rowblocked(2)
    xs = [g.get_x(c) for c in range(Cn)]
    reps = g.mg_conjugate_gradient_rowblocked(1e-30, 40, 2)
    record(out, "rowblock_96x80", xs + [g.get_x(c) for c in range(Cn)], reps)
    g.attach_comm(None)
    g.close()
    comm.close()
    # the CG passes outside multigrid
    for name, fused in (("grid_cg_fused", None), ("grid_cg_three_pass", "0")):
        os.environ.pop("CCP_GS_CG_FUSED", None)
        if fused is not None:
            os.environ["CCP_GS_CG_FUSED"] = fused
        g = capi.Grid(W, H, Cn)
        g.randomize_x(1234, 0.0, 255.0)
        g.b_from_x()
        g.randomize_x(1235, 0.0, 255.0)
        reps = g.conjugate_gradient(1e-30, 20)
        record(out, name, [g.get_x(c) for c in range(Cn)], reps)
        g.close()
    os.environ.pop("CCP_GS_CG_FUSED", None)
    rng, n = synth.rng(1), 257                              # symmetric, dominant, one empty row: stored, not a grid
    dense = np.where(rng.uniform(size=(n, n)) < 0.02, rng.uniform(-1, 1, (n, n)), 0.0)
    dense = dense + dense.T
    np.fill_diagonal(dense, np.abs(dense).sum(axis=1) + 1.0)
    dense[5, :] = 0.0
    rows, cols = np.nonzero(dense)
    r = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    m = capi.CsrMatrix().upload_compressed(dense[rows, cols], cols.astype(np.int32), r, n_cols=n)
    xt = synth.x_true(n, 1234)
    b = dense @ xt
    x1, rep1 = m.conjugate_gradient(b, 1e-30, 20)
    x2, rep2 = m.conjugate_gradient(b, 1e-30, 20, init=xt * 1e-3 + 0.25)
    record(out, "csr_cg_stored", [x1, x2], [rep1, rep2])
    m.close()
    assert sorted(out) == sorted(cases())
    with open(out_path, "w") as f:
        json.dump({"lib": os.environ.get("CCP_GS_LIB", "default"), "cases": out}, f)
    print("done", len(out), "cases; all finite:", all(v["x_finite"] for v in out.values()), flush=True)


def compare(a_path, b_path, out_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    all_ok = True
    with open(out_path, "w") as out:
        for c in cases():
            ra, rb = a["cases"][c], b["cases"][c]
            rec = {"case": c, "x_bytes_equal": ra["x_sha256"] == rb["x_sha256"], "report_bytes_equal": ra["report_hex"] == rb["report_hex"],
                   "x_finite": rb["x_finite"], "x_sha256": [h[:16] for h in rb["x_sha256"]], "reports": rb["reports"]}
            ok = rec["x_bytes_equal"] and rec["report_bytes_equal"] and rec["x_finite"]
            all_ok &= ok
            out.write(json.dumps(rec) + "\n")
            if not ok:
                print("FAIL", c, ra["reports"], rb["reports"])
    print(len(cases()), "cases:", "ALL EQUAL" if all_ok else "SOME DIFFER", f"({a['lib']} / {b['lib']})")
    return 0 if all_ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(cases()))
    elif sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:5]))
