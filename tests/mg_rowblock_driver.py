"""Child process of tests/test_gpu_mg_rowblock.py (never imported by the product): multigrid-preconditioned CG on row
blocks (ccp_grid_mg_conjugate_gradient_rowblocked, ccp_grid_mg_apply_rowblocked, ccp_grid_mg_rowblock_info) at world
size 2..8 on ONE card, every result compared with the one-block call on the whole image.

The ranks are threads of this process and CCP_GS_RCCL_LIB points libccp_gs.so at tests/cpp/libfake_rccl.so, as in
tests/rccl_threads_driver.py (whose run_ranks, system and region_mask this reuses).

usage: mg_rowblock_driver.py '<json list of cases>'   ->  one JSON line per case on stdout
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coursecomputationalphotography_amd import capi, rowblock, synth  # noqa: E402
from rccl_threads_driver import region_mask, run_ranks, system  # noqa: E402


def cuts_of(c):
    if c.get("cuts"):
        return c["cuts"]
    parts = rowblock.partition_rows(c["H"], c["world"])
    return [p[0] for p in parts] + [c["H"]]


def mask_of(c, key="mask"):
    """None, the threads driver's region (the disc mask of BASELINE configs[4] at its radii) or a small-radius disc mask."""
    m = c.get(key)
    if not m:
        return None
    if m == "region":
        return region_mask({"W": c["W"], "H": c["H"], "mask": True, "seed": c.get("seed", 4321)})
    return synth.disc_mask(c["W"], c["H"], seed=int(m)).astype(np.uint8)


def block(c, cuts, rank, mask):
    lo, hi = cuts[rank], cuts[rank + 1]
    return capi.Grid(c["W"], c["H"], c.get("C", 1), lo, hi - lo, c.get("ghost", 1), 0, mask=mask)


def errors(out, err):
    return {"ok": False, "error": [repr(e) for e in err if e is not None]}


def case_apply(c):
    """One V-cycle across the blocks: each rank's owned rows of x == the one-block mg_apply, bit for bit."""
    W, H, C_, nu = c["W"], c["H"], c.get("C", 1), c["nu"]
    mask = mask_of(c)
    g = np.random.Generator(np.random.MT19937(c.get("seed", 11)))
    bs = [g.uniform(-300.0, 300.0, (H, W)) for _ in range(C_)]
    if mask is not None:
        bs = [np.where(mask != 0, b, 0.0) for b in bs]
    whole = capi.Grid(W, H, C_, mask=mask)
    for ch in range(C_):
        whole.set_b(bs[ch], ch)
    whole.fill_x(7.0)
    whole.mg_apply(nu)
    want = np.stack([whole.get_x(ch) for ch in range(C_)])
    whole.close()
    cuts = cuts_of(c)

    def rank_fn(rank, comm):
        gb = block(c, cuts, rank, mask)
        for ch in range(C_):
            gb.set_b(bs[ch][gb.first_local_row:gb.first_local_row + gb.local_rows], ch)
        gb.fill_x(7.0)
        gb.attach_comm(comm)
        info = gb.mg_rowblock_info()
        gb.mg_apply_rowblocked(nu)
        owned = np.stack([gb.get_x_owned(ch) for ch in range(C_)])
        gb.attach_comm(None)
        gb.close()
        return owned, info

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return errors(out, err)
    got = np.concatenate([o[0] for o in out], axis=1)
    return {"ok": True, "bit_identical": bool(np.array_equal(got, want)),
            "max_abs_diff": float(np.max(np.abs(got - want))), "info": [o[1] for o in out]}


def case_info(c):
    """mg_rowblock_info on every rank."""
    cuts = cuts_of(c)

    def rank_fn(rank, comm):
        gb = block(c, cuts, rank, None)
        gb.attach_comm(comm)
        info = gb.mg_rowblock_info()
        gb.attach_comm(None)
        gb.close()
        return info

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return errors(out, err)
    whole = capi.Grid(c["W"], c["H"], 1)
    sizes = [(d.shape[1], d.shape[0]) for d, _, _ in whole.mg_levels()]
    whole.close()
    return {"ok": True, "info": out, "level_sizes": sizes}


def eps_of(c, g):
    """the case's epsilon: a fixed value, or rel * |b| (the largest channel's) from the one-block handle"""
    if "rel" in c:
        _, bb = g.residual_norm2()
        return c["rel"] * float(np.sqrt(bb.max()))
    return c["eps"]


def case_pcg(c):
    """The PCG loop across the blocks against the one-block call: x to rounding, the same report on every rank, the
    stop confirmed by the global residual.  bands: compare only these row bands (bounded host memory at full size).
    remask: after the first solve, set another mask on every rank and solve again (the hierarchy must follow it).
    sweep_after: a row-blocked sweep after the solve must refresh the stale ghost rows itself.  x0: the start value of
    x (0 without it); with it every rank also says whether its owned rows still hold x0, bit for bit (iters 0)."""
    W, H, C_, nu, iters = c["W"], c["H"], c.get("C", 1), c.get("nu", 2), c["iters"]
    mask = mask_of(c)
    bands = c.get("bands") or [[0, H]]
    x0 = c.get("x0", 0.0)
    whole = capi.Grid(W, H, C_, mask=mask)
    system(whole)
    whole.fill_x(x0)
    eps = eps_of(c, whole)
    reps_w = whole.mg_conjugate_gradient(eps, iters, nu)
    want = [np.stack([whole.get_x(ch, lo, hi - lo) for ch in range(C_)]) for lo, hi in bands]
    rep_w = [(r.iterations, r.converged, r.last_l1_step) for r in reps_w]
    want2, rep_w2 = None, None
    mask2 = mask_of(c, "remask")
    if mask2 is not None:
        whole.set_mask(mask2)
        system(whole)
        whole.fill_x(0.0)
        reps2 = whole.mg_conjugate_gradient(eps, iters, nu)
        want2 = np.stack([whole.get_x(ch) for ch in range(C_)])
        rep_w2 = [(r.iterations, r.converged, r.last_l1_step) for r in reps2]
    whole.close()
    cuts = cuts_of(c)

    def rank_fn(rank, comm):
        gb = block(c, cuts, rank, mask)
        system(gb)
        gb.fill_x(x0)
        gb.attach_comm(comm)
        reps = gb.mg_conjugate_gradient_rowblocked(eps, iters, nu)
        rr, _ = gb.residual_norm2_global()
        lo, hi = cuts[rank], cuts[rank + 1]
        mine = []
        for blo, bhi in bands:
            a, b = max(lo, blo), min(hi, bhi)
            mine.append(np.stack([gb.get_x(ch, a, b - a) for ch in range(C_)]) if a < b else None)
        res = {"reps": [(r.iterations, r.converged, r.last_l1_step) for r in reps], "rr": rr.tolist()}
        if "x0" in c:
            start = np.full((gb.get_x_owned(0).shape), x0).view(np.uint64)
            res["x_is_start"] = all(np.array_equal(gb.get_x_owned(ch).view(np.uint64), start) for ch in range(C_))
        if c.get("sweep_after"):
            gb.sweep_rowblocked(2)
            res["after"] = np.stack([gb.get_x_owned(ch) for ch in range(C_)])
        if mask2 is not None:
            gb.set_mask(mask2)
            system(gb)
            gb.fill_x(0.0)
            reps2 = gb.mg_conjugate_gradient_rowblocked(eps, iters, nu)
            res["reps2"] = [(r.iterations, r.converged, r.last_l1_step) for r in reps2]
            res["x2"] = np.stack([gb.get_x_owned(ch) for ch in range(C_)])
        gb.attach_comm(None)
        gb.close()
        return mine, res

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return errors(out, err)
    num = den = 0.0
    for i in range(len(bands)):
        got = np.concatenate([o[0][i] for o in out if o[0][i] is not None], axis=1)
        num += float(np.sum((got - want[i]) ** 2))
        den += float(np.sum(want[i] ** 2))
    res = {"ok": True, "eps": eps, "rel_diff": float(np.sqrt(num / den)), "report_one_block": rep_w,
           "report_ranks": [o[1]["reps"] for o in out], "rnorm_global": [list(np.sqrt(o[1]["rr"])) for o in out]}
    if "x0" in c:
        res["x_is_start"] = [o[1]["x_is_start"] for o in out]
    if c.get("sweep_after"):
        got_x = np.concatenate([o[0][0] for o in out], axis=1)
        ref = capi.Grid(W, H, C_, mask=mask)
        system(ref)
        for ch in range(C_):
            ref.set_x(got_x[ch], ch)
        ref.sweep(2)
        after_w = np.stack([ref.get_x(ch) for ch in range(C_)])
        ref.close()
        res["sweep_after_bit_identical"] = bool(np.array_equal(np.concatenate([o[1]["after"] for o in out], axis=1), after_w))
    if mask2 is not None:
        x2 = np.concatenate([o[1]["x2"] for o in out], axis=1)
        res["remask_rel_diff"] = float(np.linalg.norm(x2 - want2) / np.linalg.norm(want2))
        res["remask_report_one_block"] = rep_w2
        res["remask_report_ranks"] = [o[1]["reps2"] for o in out]
    return res


def case_refused(c):
    """Arguments or a partition the call cannot take: the same status on every rank, and nobody hangs.  Afterwards a
    valid call on the same handles still works (every rank issued the same collectives, i.e. none)."""
    cuts = cuts_of(c)

    def rank_fn(rank, comm):
        gb = block(c, cuts, rank, None)
        system(gb)
        gb.fill_x(0.0)
        if c.get("attach", True):
            gb.attach_comm(comm)
        status = []
        for call in c["calls"]:
            try:
                if call[0] == "pcg":
                    gb.mg_conjugate_gradient_rowblocked(1e-10, 5, call[1])
                else:
                    gb.mg_apply_rowblocked(call[1])
                status.append(0)
            except capi.CcpError as e:
                status.append(e.status)
        if c.get("attach", True):
            gb.attach_comm(None)
        gb.close()
        return status

    out, err = run_ranks(len(cuts) - 1, rank_fn)
    if any(err):
        return errors(out, err)
    return {"ok": True, "status": out}


CASES = {"apply": case_apply, "info": case_info, "pcg": case_pcg, "refused": case_refused}


def main():
    if not os.environ.get("CCP_GS_RCCL_LIB"):
        raise SystemExit("CCP_GS_RCCL_LIB must name the test transport")
    for c in json.loads(sys.argv[1]):
        try:
            res = CASES[c["kind"]](c)
        except Exception as e:  # noqa: BLE001
            res = {"ok": False, "error": repr(e)}
        print(json.dumps({"case": c, **res}), flush=True)


if __name__ == "__main__":
    main()
