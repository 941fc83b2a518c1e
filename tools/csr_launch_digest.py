#!/usr/bin/env python3
"""Launch digest of the CSR solve, product and residual entry points, to compare two builds of the library (NOTES §R24.1).

  csr_launch_digest.py --list                  the case names
  csr_launch_digest.py run CASE OUT.json       the calls of one case with the library CCP_GS_LIB names; sha256 of every result
                                               vector and the reports' bytes go to OUT.json.  Run it under `rocprofv3
                                               --kernel-trace --memory-copy-trace --output-format csv -d
                                               ROOT/trace/CASE/{parent,new} -o t --`, in a fresh process per case and
                                               library, with OUT = ROOT/res/CASE.{parent,new}.json
  csr_launch_digest.py compare ROOT            per case: the ordered dispatches (kernel name, grid, workgroup, LDS bytes), the
                                               ordered copies (direction, bytes) where they were traced, and the result bytes
                                               of the two libraries; writes ROOT/launch_digest.jsonl

Matrices: P the Poisson matrix 24x17 (408 rows), R the Laplacian of a disc mask on 96x80, S a random sparse matrix (n = 257),
T a rectangular one (apply only).  A Gauss-Seidel case runs (epsilon, cap, every) = (0.5, 600, 1), (0.5, 600, 3), (0, 13, 1),
(0, 33, 0), each on a fresh handle (a second solve on one handle would time the region twin's tiling), then (0.5, 600, 1)
from a start vector where the case name ends in _x0.  The switches are set in the environment before the upload reads them."""
import csv, glob, hashlib, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np

GS_ARGS = [(0.5, 600, 1), (0.5, 600, 3), (0.0, 13, 1), (0.0, 33, 0)]
SWITCHES = ("CCP_GS_STRUCTURED", "CCP_GS_MASKED", "CCP_GS_ONE_BLOCK", "CCP_GS_PIPELINE", "CCP_GS_CG_FUSED", "CCP_GS_ROWS_OVERLAP")
STORED = {"CCP_GS_STRUCTURED": "0"}
GROUPS = {"CCP_GS_STRUCTURED": "0", "CCP_GS_ONE_BLOCK": "0"}

# name -> (matrix, order, caller's colouring, environment, with a start vector too)
GS_CASES = {
    "gs_P_twin_colour_x0": ("P", "colour", True, {}, True),
    "gs_P_twin_index": ("P", "index", True, {}, False),
    "gs_R_twin_colour_x0": ("R", "colour", True, {}, True),
    "gs_R_twin_colour_no_colouring": ("R", "colour", False, {}, False),
    "gs_R_twin_index": ("R", "index", True, {}, False),
    "gs_R_twin_index_no_colouring": ("R", "index", False, {}, False),
    "gs_P_one_workgroup_colour": ("P", "colour", True, STORED, False),
    "gs_P_one_workgroup_index_x0": ("P", "index", True, STORED, True),
    "gs_P_pipeline_index_x0": ("P", "index", True, GROUPS, True),
    "gs_P_groups_colour_x0": ("P", "colour", True, GROUPS, True),
    "gs_P_groups_index": ("P", "index", True, dict(GROUPS, CCP_GS_PIPELINE="0"), False),
    "gs_S_colour": ("S", "colour", False, {}, False),
    "gs_S_index": ("S", "index", False, {}, False),
    "rb_gs_overlap_x0": ("R", "colour", True, {"CCP_GS_MASKED": "0"}, True),
    "rb_gs_no_overlap": ("R", "colour", True, {"CCP_GS_MASKED": "0", "CCP_GS_ROWS_OVERLAP": "0"}, False),
}
# name -> (matrix, environment)
CG_CASES = {
    "cg_P_twin": ("P", {}),
    "cg_R_fused": ("R", {"CCP_GS_MASKED": "0"}),
    "cg_R_three_pass": ("R", {"CCP_GS_MASKED": "0", "CCP_GS_CG_FUSED": "0"}),
    "jacobi_R": ("R", {"CCP_GS_MASKED": "0"}),
    "rb_cg": ("R", {"CCP_GS_MASKED": "0"}),
    "rb_jacobi": ("R", {"CCP_GS_MASKED": "0"}),
}
AR_CASES = {
    "ar_P_twin": ("P", {}),
    "ar_R_region_twin_after_a_solve": ("R", {}),
    "ar_R_stored": ("R", {"CCP_GS_MASKED": "0"}),
    "ar_S_stored": ("S", {}),
    "apply_T_rectangular": ("T", {}),
    "rb_ar": ("R", {"CCP_GS_MASKED": "0"}),
}


def cases():
    return list(GS_CASES) + list(CG_CASES) + list(AR_CASES)


def matrix(which):
    """(values, columns, row offsets, n_cols, colouring or None, number of colours)"""
    import oracle
    from coursecomputationalphotography_amd import synth
    if which == "P":
        v, c, r = synth.poisson_csr(24, 17)
        return v, c, r, len(r) - 1, oracle.grid_colour(24, 17), 2
    if which == "R":
        mask = synth.disc_mask(96, 80, seed=4321, n_discs=12, rmin=600.0, rmax=1800.0)      # 4,788 unknowns
        v, c, r, colour, _, _ = synth.masked_laplacian_csr(mask)
        return v, c, r, len(r) - 1, colour, 2
    g = synth.rng(1)
    n, nc = (257, 257) if which == "S" else (130, 211)
    dense = np.where(g.uniform(size=(n, nc)) < 0.02, g.uniform(-1, 1, (n, nc)), 0.0)
    if which == "S":                       # in the style of test_random_sparse_vs_oracle: symmetric, dominant, one empty row
        dense = dense + dense.T
        np.fill_diagonal(dense, np.abs(dense).sum(axis=1) + 1.0)
        dense[5, :] = 0.0
    rows, cols = np.nonzero(dense)
    r = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return dense[rows, cols], cols.astype(np.int32), r, nc, None, 0


def run(name, out_path):
    spec = GS_CASES.get(name) or CG_CASES.get(name) or AR_CASES[name]
    which, env = spec[0], spec[3] if name in GS_CASES else spec[1]
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    from coursecomputationalphotography_amd import capi, synth
    v, c, r, n_cols, colour, n_colours = matrix(which)
    n = len(r) - 1
    rowblock = name.startswith("rb_")
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0) if rowblock else None

    def handle(with_colouring=True):
        if rowblock:
            return capi.CsrMatrix().upload_rows(comm, 0, n, v, c, r[:-1], np.diff(r), colour, n_colours)
        m = capi.CsrMatrix().upload_compressed(v, c, r, n_cols=n_cols)
        if with_colouring and colour is not None:
            m.set_colouring(colour, n_colours)
        return m

    xt = synth.x_true(n_cols, 1234)
    b = synth.csr_apply(v, c, r, xt) * 1e-3 if which != "T" else None
    vectors, reports, paths = [], [], []

    def keep(x, rep=None):
        vectors.append(np.ascontiguousarray(x, dtype=np.float64))
        if rep is not None:
            reports.append([rep.iterations, rep.converged, rep.last_l1_step])

    if name in GS_CASES:
        _, order, with_colouring, _, with_x0 = GS_CASES[name]
        ordering = capi.ORDER_LEXICOGRAPHIC if order == "index" else capi.ORDER_MULTICOLOUR
        for eps, cap, every, x0 in [a + (None,) for a in GS_ARGS] + ([GS_ARGS[0] + (xt * 1e-3 + 0.25,)] if with_x0 else []):
            m = handle(with_colouring)
            keep(*m.gauss_seidel(b, eps, cap, x0=x0, check_every=every, ordering=ordering))
            paths.append(m.last_path())
            m.close()
    elif name in CG_CASES:
        m = handle()
        if "jacobi" in name:
            keep(*m.conjugate_gradient_jacobi(b, 1e-30, 20))
        else:
            keep(*m.conjugate_gradient(b, 1e-30, 20))
            keep(*m.conjugate_gradient(b, 1e-30, 20, init=xt * 1e-3 + 0.25))
        m.close()
    else:
        m = handle()
        if "after_a_solve" in name:
            keep(*m.gauss_seidel(b, 0.0, 9, check_every=0))
            paths.append(m.last_path())
        keep(m.apply_to_vector(xt))
        if which != "T":
            keep(np.array(m.residual_norm2(b, xt * 1e-3 + 0.25)))
        m.close()
    if comm is not None:
        comm.close()
    rep = np.array(reports, dtype=np.float64)
    res = {"case": name, "lib": os.environ.get("CCP_GS_LIB", "default"), "env": env, "paths": paths,
           "x_sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in vectors],
           "x_finite": bool(all(np.isfinite(x).all() for x in vectors)), "report_hex": rep.tobytes().hex(), "reports": rep.tolist()}
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("done", name, paths, res["reports"], flush=True)


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError((names, list(row)))


def trace(d, what):
    files = glob.glob(os.path.join(d, "**", f"*{what}.csv"), recursive=True)
    assert len(files) <= 1, (d, files)
    return list(csv.DictReader(open(files[0]))) if files else None


def dispatches(d):
    rows = trace(d, "kernel_trace")
    assert rows is not None, d
    rows.sort(key=lambda r: int(col(r, "Dispatch_Id")))
    return [(col(r, "Kernel_Name"),
             tuple(int(col(r, f"Grid_Size_{a}")) for a in "XYZ"),
             tuple(int(col(r, f"Workgroup_Size_{a}")) for a in "XYZ"),
             int(col(r, "LDS_Block_Size", "LDS_Block_Size_Bytes"))) for r in rows]


def copies(d):
    """Ordered (direction, bytes) of the traced copies; bytes is None where the profiler's table has no such column."""
    rows = trace(d, "memory_copy_trace")
    if rows is None:
        return None
    rows.sort(key=lambda r: int(col(r, "Start_Timestamp")))
    size = next((k for k in (rows[0] if rows else {}) if "byte" in k.lower() or k.lower() == "size"), None)
    return [(col(r, "Direction"), int(r[size]) if size else None) for r in rows]


def digest(lst):
    return hashlib.sha256(json.dumps(lst).encode()).hexdigest()[:16]


def compare(root):
    all_ok = True
    with open(os.path.join(root, "launch_digest.jsonl"), "w") as out:
        for c in cases():
            if not os.path.exists(os.path.join(root, "res", f"{c}.new.json")):
                print("MISSING", c)
                all_ok = False
                continue
            p, n = dispatches(os.path.join(root, "trace", c, "parent")), dispatches(os.path.join(root, "trace", c, "new"))
            cp, cn = copies(os.path.join(root, "trace", c, "parent")), copies(os.path.join(root, "trace", c, "new"))
            rp, rn = (json.load(open(os.path.join(root, "res", f"{c}.{s}.json"))) for s in ("parent", "new"))
            diffs = [(i, a, b) for i, (a, b) in enumerate(zip(p, n)) if a != b]
            rec = {"case": c, "env": rn["env"], "paths": rn["paths"], "dispatches_parent": len(p), "dispatches_new": len(n),
                   "hash_parent": digest(p), "hash_new": digest(n), "same_dispatches": len(p) == len(n) and not diffs,
                   "copies_parent": None if cp is None else len(cp), "copies_new": None if cn is None else len(cn),
                   "copy_bytes_traced": bool(cp) and cp[0][1] is not None, "same_copies": cp == cn,
                   "x_bytes_equal": rp["x_sha256"] == rn["x_sha256"], "report_bytes_equal": rp["report_hex"] == rn["report_hex"],
                   "x_finite": rn["x_finite"], "reports": rn["reports"]}
            if not rec["same_dispatches"]:
                rec["first_differences"] = [list(map(str, d)) for d in diffs[:4]]
            if not rec["same_copies"] and cp is not None and cn is not None:
                rec["first_copy_differences"] = [[i, str(a), str(b)] for i, (a, b) in enumerate(zip(cp, cn)) if a != b][:4]
            ok = rec["same_dispatches"] and rec["same_copies"] and rec["x_bytes_equal"] and rec["report_bytes_equal"]
            all_ok &= ok
            out.write(json.dumps(rec) + "\n")
            print("OK  " if ok else "FAIL", c, rec["dispatches_parent"], rec["dispatches_new"], "copies", rec["copies_parent"], rec["copies_new"],
                  rec["paths"], rec["reports"])
    print("ALL OK" if all_ok else "SOME FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(cases()))
    elif sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2]))
