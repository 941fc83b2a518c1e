#!/usr/bin/env python3
"""Multigrid-preconditioned CG (ccp_grid_mg_conjugate_gradient) on one MI355X: iterations to 1e-10 |b|, ms per PCG
iteration, ms to 1e-10, hierarchy setup ms, and GB/s on the byte model of the issue that introduced it: about 165 B per
unknown and PCG iteration (level 0 of a V-cycle ~60 B, coarse levels ~a third of that plus their coefficients, PCG
vector work ~80 B).  The model is the fused design's; the passes as built move more (NOTES.md), so the GB/s column is
a figure of merit, not a measured traffic.  One JSON line per case and precision: 16384^2, 4096^2 x 3, 752x566 x 3, the 8192^2
disc_mask region.  --precision: a comma list of f64 / f32 (capi.Grid.mg_set_precision), solved in that order on the same
handle, so f64,f32,f64,f32,f64,f32 alternates three times and shows f64's spread against itself.  first_apply_ms and apply_ms are the wall times of the first and
the second ccp_grid_mg_apply after the hierarchy is built (one V-cycle per channel; in f32 the first also narrows the
coefficients, which setup_ms and the solve's own timing leave out).  --channels: a comma list of sequential / batched
(capi.Grid.mg_set_channels), the outer alternation on the same handle: every entry runs the whole --precision list.  A
batched solve reports the elapsed time of the whole solve in every channel, so its time is one report's seconds, not
their sum; ms_per_pcg_iteration divides by the updates summed over the channels in both modes.  A list of `sequential`
alone never calls the setter, so it also runs on a library without it."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
from coursecomputationalphotography_amd import capi, synth

MODEL_B = 165.0
CASES = {"16384sq": (16384, 16384, 1, False), "4096sq_x3": (4096, 4096, 3, False), "752x566_x3": (752, 566, 3, False),
         "disc8192": (8192, 8192, 1, True)}

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default=",".join(CASES))
ap.add_argument("--sweeps", type=int, default=2)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--max-iterations", type=int, default=50)
ap.add_argument("--precision", default="f64", help="comma list of f64 / f32, in the order to run them")
ap.add_argument("--channels", default="sequential", help="comma list of sequential / batched, in the order to run them")
a = ap.parse_args()
modes = a.channels.split(",")
for m in modes:
    if m not in capi.MG_CHANNELS:
        ap.error(f"--channels: {m!r} is not one of {sorted(capi.MG_CHANNELS)}")
set_mode = modes != ["sequential"] * len(modes)
precisions = a.precision.split(",")
for p in precisions:
    if p not in capi.MG_PRECISIONS:
        ap.error(f"--precision: {p!r} is not one of {sorted(capi.MG_PRECISIONS)}")
for name in a.cases.split(","):
    W, H, C, masked = CASES[name]
    mask = synth.disc_mask(W, H, seed=4321) if masked else None
    g = capi.Grid(W, H, C, mask=mask)
    n = int(mask.sum()) if masked else W * H
    g.randomize_x(1234, 0.0, 255.0)
    g.b_from_x()
    g.synchronize()
    for run, (mode, precision) in enumerate((m, p) for m in modes for p in precisions):
        g.mg_set_precision(precision)
        if set_mode:
            g.mg_set_channels(mode)
        t0 = time.perf_counter()
        nl = ctypes.c_int32()                                       # the first MG call builds the hierarchy
        capi.check(g.L.ccp_grid_mg_level(g.h, 0, ctypes.byref(nl), None, None, None, None, None), "ccp_grid_mg_level")
        g.synchronize()
        setup_ms = (time.perf_counter() - t0) * 1e3
        # one V-cycle per channel, twice: the first also narrows the coefficients in f32 (x is zeroed below)
        t0 = time.perf_counter()
        g.mg_apply(a.sweeps)
        first_apply_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        g.mg_apply(a.sweeps)
        apply_ms = (time.perf_counter() - t0) * 1e3
        best = None
        for _ in range(a.repeat):
            g.fill_x(0.0)
            _, bb = g.residual_norm2()
            eps = 1e-10 * float(np.sqrt(bb.max()))
            reps = g.mg_conjugate_gradient(eps, a.max_iterations, a.sweeps)
            secs = reps[0].seconds if mode == "batched" else sum(r.seconds for r in reps)
            if best is None or secs < best[0]:
                best = (secs, [r.iterations for r in reps], [bool(r.converged) for r in reps])
        rr, bb = g.residual_norm2()
        secs, its, conv = best
        # a solve of `it` counted iterations runs it + 1 updates (and as many V-cycles, the initial one included)
        updates = sum(i + 1 for i in its)
        ms_per_iter = secs * 1e3 / updates
        print(json.dumps({"case": name, "precision": precision, "mg_channels": mode, "run": run, "max_iterations": a.max_iterations, "width": W, "height": H, "channels": C, "unknowns_per_channel": n, "levels": nl.value,
                          "smoothing_sweeps": a.sweeps, "iterations": its, "converged": conv, "ms_to_1e-10": secs * 1e3,
                          "ms_per_pcg_iteration": ms_per_iter, "setup_ms": setup_ms,
                          "first_apply_ms": first_apply_ms, "apply_ms": apply_ms, "model_GBps": MODEL_B * n * updates / secs / 1e9,
                          "rel_residual": float(np.sqrt(rr / bb).max())}), flush=True)
    g.close()
