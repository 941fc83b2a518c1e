#!/usr/bin/env python3
"""Weighted grid handles with fixed pixels on one MI355X: a screened system (lambda = 1e-2, wx = wy = 1, rescaled
hierarchy) whose free region is a central ellipse, every pixel outside it fixed, at 4096^2 x 3 and 16384^2, beside the
same handle with no fixed pixels.  The two kinds alternate in one process (--order, default free,fixed three times over):
each run installs its operator (set_weights_tensor with or without the mask: the formation pass, timed with its
read-back), assembles b (timed) and solves by MG-PCG to 1e-10 |b| or --max-iterations, whichever comes first.  One JSON
line per run, then one summary line per case: the best ms per PCG iteration of each kind, the spread of the runs of each
kind against themselves, and the best set-up times.  With a small --max-iterations both kinds do the same number of
iterations, which is what makes their ms per iteration comparable."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"screened_4096sq_x3": (4096, 4096, 3), "screened_16384sq": (16384, 16384, 1)}


def ellipse_outside(W, H, dev):
    """u8 H x W, 1 outside the central ellipse with half-axes 0.4 W and 0.4 H."""
    y = (torch.arange(H, device=dev, dtype=torch.float32) - (H - 1) / 2) / (0.4 * H)
    x = (torch.arange(W, device=dev, dtype=torch.float32) - (W - 1) / 2) / (0.4 * W)
    return ((y * y)[:, None] + (x * x)[None, :] >= 1.0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--order", default="free,fixed,free,fixed,free,fixed", help="comma list of free / fixed, in the order to run them")
    ap.add_argument("--hierarchy", default="rescaled")
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--max-iterations", type=int, default=200)
    a = ap.parse_args()
    order = a.order.split(",")
    for k in order:
        if k not in ("free", "fixed"):
            ap.error(f"--order: {k!r} is not free or fixed")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, C = CASES[name]
        gen = torch.Generator(device=dev).manual_seed(7)
        gx = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
        gy = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
        f = torch.rand((H, W, C), generator=gen, device=dev) * 255.0
        values = (torch.rand((H, W, C), generator=gen, device=dev) * 255.0).to(torch.uint8)
        mask = ellipse_outside(W, H, dev)
        lam = torch.tensor(1e-2, dtype=torch.float64, device=dev).expand(H, W)
        g = capi.Grid(W, H, C, weighted=True)
        g.mg_set_hierarchy(a.hierarchy)
        runs = {"free": [], "fixed": []}
        for run, kind in enumerate(order):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.set_weights_tensor(None, None, lam, fixed=mask if kind == "fixed" else None)     # synchronises: the verdict
            form_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            if kind == "fixed":
                g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=True)
            else:
                g.assemble_weighted_rhs_tensor(gx, gy, f, init_x=True)
            torch.cuda.synchronize()
            rhs_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            nl = ctypes.c_int32()                                       # the first MG call on an operator builds its hierarchy
            capi.check(g.L.ccp_grid_mg_level(g.h, 0, ctypes.byref(nl), None, None, None, None, None), "ccp_grid_mg_level")
            g.synchronize()
            hierarchy_ms = (time.perf_counter() - t0) * 1e3
            _, bb = g.residual_norm2()
            eps = 1e-10 * float(np.sqrt(bb.max()))
            reps = g.mg_conjugate_gradient(eps, a.max_iterations, a.sweeps)
            secs = sum(r.seconds for r in reps)
            its = [r.iterations for r in reps]
            updates = sum(i + 1 for i in its)                           # as tools/mg_bench.py counts them
            rr, bb = g.residual_norm2()
            rec = {"case": name, "width": W, "height": H, "channels": C, "kind": kind, "run": run, "hierarchy": a.hierarchy,
                   "constraint_info": g.constraint_info(), "max_iterations": a.max_iterations, "iterations": its,
                   "converged": [bool(r.converged) for r in reps], "ms_solve": secs * 1e3, "ms_per_pcg_iteration": secs * 1e3 / updates,
                   "form_ms": form_ms, "rhs_ms": rhs_ms, "hierarchy_ms": hierarchy_ms, "rel_residual": float(np.sqrt(rr / bb).max())}
            runs[kind].append(rec)
            print(json.dumps(rec), flush=True)
        summary = {"case": name, "summary": True, "max_iterations": a.max_iterations}
        for kind, rs in runs.items():
            if rs:
                per = [r["ms_per_pcg_iteration"] for r in rs]
                summary[kind] = {"runs": len(rs), "best_ms_per_pcg_iteration": min(per), "spread_ms_per_pcg_iteration": max(per) - min(per),
                                 "iterations": rs[0]["iterations"], "best_form_ms": min(r["form_ms"] for r in rs),
                                 "best_rhs_ms": min(r["rhs_ms"] for r in rs)}
        print(json.dumps(summary), flush=True)
        g.close()
        del gx, gy, f, values, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
