#!/usr/bin/env python3
"""Weighted grid handles (CCP_GRID_WEIGHTED) on one MI355X: MG-PCG iterations and milliseconds to 1e-10 |b| for a
screened Poisson system (lambda = 1e-2, wx = wy = 1) at 16384^2, WLS edge-preserving smoothing (Farbman et al. 2008:
lambda 1, alpha 1.2) at 4096^2 x 3 and at the reference's image size 752x566 x 3, and the structured handle's MG-PCG at
16384^2 beside them (ms per PCG iteration: the weighted level 0 reads its 24 B/px of stored coefficients).  One JSON
line per case and hierarchy kind (--hierarchy: a comma list of galerkin / rescaled, solved in that order on the same handle;
the default runs both, and a list such as galerkin,galerkin,rescaled measures the spread of one kind against itself beside
the difference between the kinds), as tools/mg_bench.py.  --precision: a comma list of f64 / f32 (capi.Grid.mg_set_precision),
alternated on the same handle in the same way: every entry runs the whole --hierarchy list, so f64,f32,f64,f32,f64,f32
gives three alternations and f64 against itself as the noise floor.  first_apply_ms and apply_ms are the wall times of
the first and the second ccp_grid_mg_apply after the hierarchy is built (one V-cycle per channel; in f32 the first also
narrows the coefficients, which setup_ms and the solve's own timing leave out).  --channels: a comma list of sequential /
batched (capi.Grid.mg_set_channels), the outermost alternation on the same handle: every entry runs the whole --precision x
--hierarchy list.  A batched solve reports the elapsed time of the whole solve in every channel, so its time is one
report's seconds, not their sum; ms_per_pcg_iteration divides by the updates summed over the channels in both modes (ms
per channel-iteration).  A list of `sequential` alone never calls the setter, so it also runs on a library without it.
--smoother: a comma list of point / line (capi.Grid.mg_set_smoother), outermost of all, alternated on the same handle in the
same way: point,line,point,line,point,line gives three alternations and point against itself as the noise floor; a list
of `point` alone never calls the setter.  --sweeps 0 (the default) is the smoother's own default: 2 point sweeps, 1 line
sweep.  With --max-iterations below the count either smoother needs, ms_per_pcg_iteration compares them at equal counts.
The screened and structured systems are manufactured (b = A x, x uniform
[0, 255)); the WLS systems smooth a synthetic image of flat patches with edges and noise, built on the device."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi, tensor_ops

CASES = {"screened_16384sq": (16384, 16384, 1, "screened"), "wls_4096sq_x3": (4096, 4096, 3, "wls"),
         "wls_752x566_x3": (752, 566, 3, "wls"), "structured_16384sq": (16384, 16384, 1, "structured")}
MORE_CASES = {"screened_4096sq_x3": (4096, 4096, 3, "screened")}   # by name only: not part of the default list


def image(W, H, C, dev):
    """Flat patches of 16 px with hard edges plus a little noise, u8."""
    g = torch.Generator(device=dev).manual_seed(7)
    patches = torch.rand((H // 16 + 1, W // 16 + 1, C), generator=g, device=dev)
    img = patches.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W] * 230.0
    img = img + 25.0 * torch.rand((H, W, C), generator=g, device=dev)
    return img.clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--hierarchy", default="galerkin,rescaled", help="comma list of galerkin / rescaled, in the order to run them")
    ap.add_argument("--precision", default="f64", help="comma list of f64 / f32, in the order to run them")
    ap.add_argument("--channels", default="sequential", help="comma list of sequential / batched, in the order to run them")
    ap.add_argument("--smoother", default="point", help="comma list of point / line, in the order to run them")
    ap.add_argument("--sweeps", type=int, default=0, help="0: the smoother's default, 2 point sweeps or 1 line sweep")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=200)
    a = ap.parse_args()
    kinds = a.hierarchy.split(",")
    for k in kinds:
        if k not in capi.MG_HIERARCHIES:
            ap.error(f"--hierarchy: {k!r} is not one of {sorted(capi.MG_HIERARCHIES)}")
    precisions = a.precision.split(",")
    for p in precisions:
        if p not in capi.MG_PRECISIONS:
            ap.error(f"--precision: {p!r} is not one of {sorted(capi.MG_PRECISIONS)}")
    modes = a.channels.split(",")
    for m in modes:
        if m not in capi.MG_CHANNELS:
            ap.error(f"--channels: {m!r} is not one of {sorted(capi.MG_CHANNELS)}")
    set_mode = modes != ["sequential"] * len(modes)
    smoothers = a.smoother.split(",")
    for sm in smoothers:
        if sm not in capi.MG_SMOOTHERS:
            ap.error(f"--smoother: {sm!r} is not one of {sorted(capi.MG_SMOOTHERS)}")
    set_smoother = smoothers != ["point"] * len(smoothers)
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, C, kind = {**CASES, **MORE_CASES}[name]
        g = capi.Grid(W, H, C, weighted=kind != "structured")
        f = None
        if kind == "screened":
            lam = torch.tensor(1e-2, dtype=torch.float64, device=dev).expand(H, W)
            g.set_weights_tensor(None, None, lam)
        elif kind == "wls":
            f = image(W, H, C, dev)
            wx, wy = tensor_ops.wls_weights(f, lam=1.0, alpha=1.2, eps=1e-4)
            g.set_weights_tensor(wx, wy, torch.tensor(1.0, dtype=torch.float64, device=dev).expand(H, W))
            g.assemble_weighted_rhs_tensor(None, None, f, init_x=True)
            torch.cuda.synchronize()
        if f is None:
            g.randomize_x(1234, 0.0, 255.0)
            g.b_from_x()
        g.synchronize()
        # a structured handle has the one hierarchy
        runs = [(sm, m, p, h) for sm in smoothers for m in modes for p in precisions for h in (kinds if kind != "structured" else ["galerkin"])]
        for run, (smoother, mode, precision, hierarchy) in enumerate(runs):
            if set_smoother:
                g.mg_set_smoother(smoother)
            if kind != "structured":
                g.mg_set_hierarchy(hierarchy)
            g.mg_set_precision(precision)
            if set_mode:
                g.mg_set_channels(mode)
            t0 = time.perf_counter()
            nl = ctypes.c_int32()                                   # the first MG call of a kind builds its hierarchy
            capi.check(g.L.ccp_grid_mg_level(g.h, 0, ctypes.byref(nl), None, None, None, None, None), "ccp_grid_mg_level")
            g.synchronize()                                         # (f32: the coefficients are narrowed at the first solve)
            setup_ms = (time.perf_counter() - t0) * 1e3
            # one V-cycle per channel, twice: the first also narrows the coefficients in f32 (x is set anew below)
            t0 = time.perf_counter()
            g.mg_apply(a.sweeps)
            first_apply_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            g.mg_apply(a.sweeps)
            apply_ms = (time.perf_counter() - t0) * 1e3
            best = None
            for _ in range(a.repeat):
                if f is None:
                    g.fill_x(0.0)
                else:
                    g.assemble_weighted_rhs_tensor(None, None, f, init_x=True)
                    torch.cuda.synchronize()
                _, bb = g.residual_norm2()
                eps = 1e-10 * float(np.sqrt(bb.max()))
                reps = g.mg_conjugate_gradient(eps, a.max_iterations, a.sweeps)
                secs = reps[0].seconds if mode == "batched" else sum(r.seconds for r in reps)
                if best is None or secs < best[0]:
                    best = (secs, [r.iterations for r in reps], [bool(r.converged) for r in reps])
            rr, bb = g.residual_norm2()
            secs, its, conv = best
            updates = sum(i + 1 for i in its)                       # as tools/mg_bench.py counts them
            print(json.dumps({"case": name, "width": W, "height": H, "channels": C, "kind": kind, "hierarchy": hierarchy, "precision": precision, "mg_channels": mode, "smoother": smoother, "run": run,
                              "levels": nl.value, "smoothing_sweeps": a.sweeps or (1 if smoother == "line" else 2), "max_iterations": a.max_iterations, "iterations": its, "converged": conv,
                              "ms_to_1e-10": secs * 1e3, "ms_per_pcg_iteration": secs * 1e3 / updates, "setup_ms": setup_ms,
                              "first_apply_ms": first_apply_ms, "apply_ms": apply_ms, "rel_residual": float(np.sqrt(rr / bb).max())}), flush=True)
        g.close()


if __name__ == "__main__":
    main()
