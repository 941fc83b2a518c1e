"""Child process of tests/test_gpu_region_blend.py (never imported by the product): the region blend entry points on
row blocks (ccp_grid_assemble_region_rhs, ccp_grid_assemble_clone, ccp_grid_store_u8_composite), every block fed
the whole canvas, every result compared with the one-block handle on the whole canvas.

The ranks are threads of this process and CCP_GS_RCCL_LIB points libccp_gs.so at tests/cpp/libfake_rccl.so, as in
tests/mg_rowblock_driver.py.

usage: blend_rowblock_driver.py '<json list of cases>'   ->  one JSON line per case on stdout
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coursecomputationalphotography_amd import capi  # noqa: E402
from blend_helpers import holey_mask  # noqa: E402
from rccl_threads_driver import run_ranks  # noqa: E402


def inputs(c):
    """The case's mask and images: a holey region clear of the border, a smooth canvas, a second image (the clone
    source), and float32 forward differences of that second image as the guidance field."""
    W, H, C_ = c["W"], c["H"], c.get("C", 3)
    g = np.random.Generator(np.random.MT19937(c.get("seed", 3)))
    mask = holey_mask(W, H, seed=c.get("seed", 3))
    yy, xx = np.mgrid[0:H, 0:W]
    canvas = np.stack([128 + 100 * np.sin(xx / (9.0 + k) + yy / (13.0 + k)) for k in range(C_)], axis=-1)
    canvas = np.clip(canvas + g.uniform(-8, 8, canvas.shape), 0, 255).astype(np.uint8)
    src = g.integers(0, 256, (H, W, C_), dtype=np.uint8)
    v = src.astype(np.int32)
    gx = np.zeros((H, W, C_), dtype=np.float32)
    gy = np.zeros((H, W, C_), dtype=np.float32)
    gx[:, :-1] = v[:, 1:] - v[:, :-1]
    gy[:-1, :] = v[1:, :] - v[:-1, :]
    return mask, canvas, src, gx, gy


def assemble(g, c, canvas, src, gx, gy):
    if c["form"] == "field":
        g.assemble_region_rhs(gx, gy, canvas, init_x=True)
    else:
        g.assemble_clone(src, canvas, mixed=c["form"] == "mixed", init=1)


def planes(g, which, C_):
    get = g.get_b if which == "b" else g.get_x
    return np.stack([get(ch) for ch in range(C_)])


def case_blend(c):
    W, H, C_, cuts = c["W"], c["H"], c.get("C", 3), c["cuts"]
    iters, ghost = c.get("iters", 40), c.get("ghost", 8)
    mask, canvas, src, gx, gy = inputs(c)
    whole = capi.Grid(W, H, C_, mask=mask)
    assemble(whole, c, canvas, src, gx, gy)
    b_w, x_w = planes(whole, "b", C_), planes(whole, "x", C_)
    whole.sweep(iters)
    comp_w = whole.store_u8_composite(canvas)
    _, bb = whole.residual_norm2()
    eps = 1e-10 * float(np.sqrt(bb.max()))
    assemble(whole, c, canvas, src, gx, gy)
    reps_w = whole.mg_conjugate_gradient(eps, 200)
    xs_w = planes(whole, "x", C_)
    whole.close()

    def rank_fn(rank, comm):
        lo, hi = cuts[rank], cuts[rank + 1]
        gb = capi.Grid(W, H, C_, lo, hi - lo, ghost, 0, mask=mask)
        assemble(gb, c, canvas, src, gx, gy)
        r0 = gb.first_local_row
        rows = slice(r0, r0 + gb.local_rows)
        same_b = bool(np.array_equal(planes(gb, "b", C_), b_w[:, rows]))
        same_x = bool(np.array_equal(planes(gb, "x", C_), x_w[:, rows]))
        gb.attach_comm(comm)
        gb.sweep_rowblocked(iters)
        comp = gb.store_u8_composite(canvas)
        assemble(gb, c, canvas, src, gx, gy)
        reps = gb.mg_conjugate_gradient_rowblocked(eps, 200)
        xs = np.stack([gb.get_x_owned(ch) for ch in range(C_)])
        gb.attach_comm(None)
        gb.close()
        return {"local_rows": [r0, r0 + gb.local_rows], "b_equal": same_b, "x_equal": same_x,
                "composite_owned_equal": bool(np.array_equal(comp[lo:hi], comp_w[lo:hi])),
                "composite_rest_untouched": bool(not comp[:lo].any() and not comp[hi:].any()),
                "iterations": [r.iterations for r in reps]}, xs

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return {"ok": False, "error": [repr(e) for e in err if e is not None]}
    xs = np.concatenate([o[1] for o in out], axis=1)
    return {"ok": True, "ranks": [o[0] for o in out], "iterations_one_block": [r.iterations for r in reps_w],
            "mg_rel_diff": float(np.linalg.norm(xs - xs_w) / np.linalg.norm(xs_w))}


def main():
    if not os.environ.get("CCP_GS_RCCL_LIB"):
        raise SystemExit("CCP_GS_RCCL_LIB must name the test transport")
    for c in json.loads(sys.argv[1]):
        try:
            res = case_blend(c)
        except Exception as e:  # noqa: BLE001 - reported to the parent
            res = {"ok": False, "error": repr(e)}
        print(json.dumps({"case": c, **res}), flush=True)


if __name__ == "__main__":
    main()
