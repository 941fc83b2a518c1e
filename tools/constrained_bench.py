#!/usr/bin/env python3
"""Weighted grid handles with fixed pixels on one MI355X: a screened system (lambda = 1e-2, wx = wy = 1, rescaled
hierarchy) whose free region is a central ellipse, every pixel outside it fixed, at 4096^2 x 3 and 16384^2, beside the
same handle with no fixed pixels.  The two kinds alternate in one process (--order, default free,fixed three times over):
each run installs its operator (set_weights_tensor with or without the mask: the formation pass, timed with its
read-back), assembles b (timed) and solves by MG-PCG to 1e-10 |b| or --max-iterations, whichever comes first.  One JSON
line per run, then one summary line per case: the best ms per PCG iteration of each kind, the spread of the runs of each
kind against themselves, and the best set-up times.  With a small --max-iterations both kinds do the same number of
iterations, which is what makes their ms per iteration comparable.
--smoother: a comma list of point / line (capi.Grid.mg_set_smoother); every entry runs the whole --order list on the same
handle, so point,line,point,line alternates the two.  --sweeps 0 is the smoother's default (2 point sweeps, 1 line
sweep).  The sparse-anchor cases (--cases anchors_752x566_x3,anchors_4096sq: not in the default list) interpolate from the
pixels [8::32, 8::32] alone: the WLS weights of tools/weighted_bench.py's image, lambda = 0, the anchors fixed at the
image's values; without the anchors that system is singular, so these cases run the `fixed` entries of --order only."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi, tensor_ops

CASES = {"screened_4096sq_x3": (4096, 4096, 3), "screened_16384sq": (16384, 16384, 1)}
ANCHOR_CASES = {"anchors_752x566_x3": (752, 566, 3), "anchors_4096sq": (4096, 4096, 1)}


def image(W, H, C, dev):
    """tools/weighted_bench.py's image: flat patches of 16 px with hard edges plus a little noise, u8."""
    g = torch.Generator(device=dev).manual_seed(7)
    patches = torch.rand((H // 16 + 1, W // 16 + 1, C), generator=g, device=dev)
    img = patches.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W] * 230.0
    img = img + 25.0 * torch.rand((H, W, C), generator=g, device=dev)
    return img.clamp(0, 255).to(torch.uint8)


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
    ap.add_argument("--smoother", default="point", help="comma list of point / line; every entry runs the whole --order list")
    ap.add_argument("--sweeps", type=int, default=2, help="0: the smoother's default, 2 point sweeps or 1 line sweep")
    ap.add_argument("--max-iterations", type=int, default=200)
    a = ap.parse_args()
    order = a.order.split(",")
    for k in order:
        if k not in ("free", "fixed"):
            ap.error(f"--order: {k!r} is not free or fixed")
    smoothers = a.smoother.split(",")
    for sm in smoothers:
        if sm not in capi.MG_SMOOTHERS:
            ap.error(f"--smoother: {sm!r} is not one of {sorted(capi.MG_SMOOTHERS)}")
    set_smoother = smoothers != ["point"] * len(smoothers)
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, C = {**CASES, **ANCHOR_CASES}[name]
        anchors = name in ANCHOR_CASES
        gen = torch.Generator(device=dev).manual_seed(7)
        gx = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
        gy = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
        f = torch.rand((H, W, C), generator=gen, device=dev) * 255.0
        values = (torch.rand((H, W, C), generator=gen, device=dev) * 255.0).to(torch.uint8)
        mask = ellipse_outside(W, H, dev)
        lam = torch.tensor(1e-2, dtype=torch.float64, device=dev).expand(H, W)
        wx = wy = None
        if anchors:
            values = image(W, H, C, dev)
            wx, wy = tensor_ops.wls_weights(values, lam=1.0, alpha=1.2, eps=1e-4)
            mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
            mask[8::32, 8::32] = 1
            gx = gy = f = lam = None
        g = capi.Grid(W, H, C, weighted=True)
        g.mg_set_hierarchy(a.hierarchy)
        runs = {}
        plan = [(sm, kind) for sm in smoothers for kind in order if not (anchors and kind == "free")]
        for run, (smoother, kind) in enumerate(plan):
            if set_smoother:
                g.mg_set_smoother(smoother)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.set_weights_tensor(wx, wy, lam, fixed=mask if kind == "fixed" else None)     # synchronises: the verdict
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
            rec = {"case": name, "width": W, "height": H, "channels": C, "kind": kind, "smoother": smoother, "run": run, "hierarchy": a.hierarchy,
                   "smoothing_sweeps": a.sweeps or (1 if smoother == "line" else 2),
                   "constraint_info": g.constraint_info(), "max_iterations": a.max_iterations, "iterations": its,
                   "converged": [bool(r.converged) for r in reps], "ms_solve": secs * 1e3, "ms_per_pcg_iteration": secs * 1e3 / updates,
                   "form_ms": form_ms, "rhs_ms": rhs_ms, "hierarchy_ms": hierarchy_ms, "rel_residual": float(np.sqrt(rr / bb).max())}
            runs.setdefault(kind if not set_smoother else f"{kind}_{smoother}", []).append(rec)
            print(json.dumps(rec), flush=True)
        summary = {"case": name, "summary": True, "max_iterations": a.max_iterations}
        for kind, rs in runs.items():
            if rs:
                per = [r["ms_per_pcg_iteration"] for r in rs]
                summary[kind] = {"runs": len(rs), "best_ms_per_pcg_iteration": min(per), "spread_ms_per_pcg_iteration": max(per) - min(per),
                                 "iterations": rs[0]["iterations"], "best_ms_solve": min(r["ms_solve"] for r in rs),
                                 "spread_ms_solve": max(r["ms_solve"] for r in rs) - min(r["ms_solve"] for r in rs), "best_form_ms": min(r["form_ms"] for r in rs),
                                 "best_rhs_ms": min(r["rhs_ms"] for r in rs)}
        print(json.dumps(summary), flush=True)
        g.close()
        del gx, gy, f, values, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
