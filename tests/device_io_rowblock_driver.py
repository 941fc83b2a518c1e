"""Child process of tests/test_gpu_device_io.py (never imported by the product): the device hand-off on row blocks.
Every block is fed whole-canvas tensors (assembly, composite) or global rows (set / get), and each result is compared
with the block's host twin and with the one-block handle.

The ranks are threads of this process and CCP_GS_RCCL_LIB points libccp_gs.so at tests/cpp/libfake_rccl.so, as in
tests/blend_rowblock_driver.py.

usage: device_io_rowblock_driver.py '<json list of cases>'   ->  one JSON line per case on stdout
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coursecomputationalphotography_amd import capi  # noqa: E402
from blend_rowblock_driver import inputs  # noqa: E402
from rccl_threads_driver import run_ranks  # noqa: E402

DEV = torch.device("cuda", 0)


def view(a, layout):
    H, W, C = a.shape
    if layout == "planar":
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)
    if layout == "window":
        big = torch.zeros((H + 2, W + 3, C), dtype=torch.from_numpy(a[:1, :1]).dtype, device=DEV)
        big[1:1 + H, 1:1 + W] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return big[1:1 + H, 1:1 + W]
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def planes(g, which, C_):
    get = g.get_b if which == "b" else g.get_x
    return np.stack([get(ch) for ch in range(C_)])


def assemble(g, c, canvas, src, gx, gy, tensors):
    if tensors is not None:
        tc, ts, tgx, tgy = tensors
        if c["form"] == "field":
            g.assemble_region_rhs_tensor(tgx, tgy, tc, init_x=True)
        else:
            g.assemble_clone_tensor(ts, tc, mixed=c["form"] == "mixed", init=1)
    elif c["form"] == "field":
        g.assemble_region_rhs(gx, gy, canvas, init_x=True)
    else:
        g.assemble_clone(src, canvas, mixed=c["form"] == "mixed", init=1)


def case(c):
    W, H, C_, cuts, lay = c["W"], c["H"], c.get("C", 3), c["cuts"], c["layout"]
    iters, ghost = c.get("iters", 40), c.get("ghost", 8)
    mask, canvas, src, gx, gy = inputs(c)
    canvas, src, gx, gy = (a.reshape(H, W, C_) for a in (canvas, src, gx, gy))
    tensors = tuple(view(a, lay) for a in (canvas, src, gx, gy))
    whole = capi.Grid(W, H, C_, mask=mask)
    assemble(whole, c, canvas, src, gx, gy, None)
    b_w, x_w = planes(whole, "b", C_), planes(whole, "x", C_)
    whole.sweep(iters)
    comp_w = whole.store_u8_composite(canvas)
    whole.close()
    rng = np.random.default_rng(c["seed"])
    field = rng.uniform(-9, 9, (H, W, C_))

    def rank_fn(rank, comm):
        lo, hi = cuts[rank], cuts[rank + 1]
        gd = capi.Grid(W, H, C_, lo, hi - lo, ghost, 0, mask=mask)
        gh = capi.Grid(W, H, C_, lo, hi - lo, ghost, 0, mask=mask)
        r0 = gd.first_local_row
        rows = slice(r0, r0 + gd.local_rows)
        # set / get on global rows, ghosts included
        gd.set_b_tensor(view(field[rows], lay), first_row=r0)
        for ch in range(C_):
            gh.set_b(field[rows, :, ch], ch, first_row=r0)
        got = gd.get_b_tensor(first_row=r0, n_rows=gd.local_rows).cpu().numpy()
        same_set = bool(np.array_equal(planes(gd, "b", C_), planes(gh, "b", C_))
                        and np.array_equal(np.moveaxis(got, -1, 0), planes(gh, "b", C_)))
        assemble(gd, c, canvas, src, gx, gy, tensors)
        torch.cuda.synchronize()
        same_b = bool(np.array_equal(planes(gd, "b", C_), b_w[:, rows]))
        same_x = bool(np.array_equal(planes(gd, "x", C_), x_w[:, rows]))
        gd.attach_comm(comm)
        gd.sweep_rowblocked(iters)
        comp = gd.store_u8_composite_tensor(tensors[0]).cpu().numpy()
        gd.attach_comm(None)
        gd.close()
        gh.close()
        return {"local_rows": [r0, r0 + gd.local_rows], "set_get_equal": same_set, "b_equal": same_b, "x_equal": same_x,
                "composite_owned_equal": bool(np.array_equal(comp[lo:hi], comp_w[lo:hi])),
                "composite_rest_untouched": bool(not comp[:lo].any() and not comp[hi:].any())}

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return {"ok": False, "error": [repr(e) for e in err if e is not None]}
    return {"ok": True, "ranks": out}


def main():
    if not os.environ.get("CCP_GS_RCCL_LIB"):
        raise SystemExit("CCP_GS_RCCL_LIB must name the test transport")
    for c in json.loads(sys.argv[1]):
        try:
            res = case(c)
        except Exception as e:  # noqa: BLE001 - reported to the parent
            res = {"ok": False, "error": repr(e)}
        print(json.dumps({"case": c, **res}), flush=True)


if __name__ == "__main__":
    main()
