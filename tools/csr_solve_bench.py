#!/usr/bin/env python3
"""The CSR entry points whose host code NOTES §R24.1 touched, at launch-bound shapes.  The 512^2 Poisson matrix kept on the stored
matrix (CCP_GS_STRUCTURED=0) in index order: the pipelined level schedule (CCP_GS_ONE_BLOCK=0, or the one-workgroup kernel would
take it), 64 sweeps with the rule after every sweep and with none, and the per-group loop (CCP_GS_PIPELINE=0 too), 20 sweeps.  The
Laplacian of a 2048^2 disc mask: the stored matrix in colour order (CCP_GS_MASKED=0) and the region twin, 50 sweeps with the rule
after every sweep; stored CG, fused and Jacobi, 50 iterations.  A product and a residual on a twin and on the stored matrix.
Per case: median, min and max over 7 calls (after warm ones) of the call's wall time and, for the solves, of report.seconds.
CCP_GS_LIB chooses the build; alternate two builds in one command to compare them.  One JSON line per case."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
from coursecomputationalphotography_amd import capi, synth

REPEAT = 7
SWITCHES = ("CCP_GS_STRUCTURED", "CCP_GS_MASKED", "CCP_GS_ONE_BLOCK", "CCP_GS_PIPELINE")


def handle(v, c, r, colour, env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)                       # (read by the upload)
    m = capi.CsrMatrix().upload_compressed(v, c, r)
    if colour is not None:
        m.set_colouring(colour, 2)
    return m


def timed(name, fn, warm=1):
    wall, own, rep = [], [], None
    for k in range(warm + REPEAT):
        t0 = time.perf_counter()
        rep = fn()
        t1 = time.perf_counter()
        if k >= warm:
            wall.append(t1 - t0)
            if hasattr(rep, "seconds"):
                own.append(rep.seconds)
    rec = {"case": name, "wall_ms_median": 1e3 * statistics.median(wall), "wall_ms_min": 1e3 * min(wall), "wall_ms_max": 1e3 * max(wall)}
    if own:
        rec.update(iterations=rep.iterations, ms_median=1e3 * statistics.median(own), ms_min=1e3 * min(own), ms_max=1e3 * max(own))
    print(json.dumps(rec), flush=True)


def solves(m, b, out, cases):
    for name, fn in cases:
        timed(name, lambda: fn(m, b, out)[1], warm=2)          # (the region twin times its tiling at the second solve)


LEX = capi.ORDER_LEXICOGRAPHIC
W = 512
v, c, r = synth.poisson_csr(W, W)
n = len(r) - 1
xt = synth.x_true(n, 4321)
b = synth.csr_apply(v, c, r, xt)
out = np.empty(n)
m = handle(v, c, r, None, {"CCP_GS_STRUCTURED": "0", "CCP_GS_ONE_BLOCK": "0"})
solves(m, b, out, [("poisson512_pipeline_64_every_sweep", lambda m, b, o: m.gauss_seidel(b, 1e-300, 64, check_every=1, ordering=LEX, out=o)),
                   ("poisson512_pipeline_64_no_rule", lambda m, b, o: m.gauss_seidel(b, 0.0, 64, check_every=0, ordering=LEX, out=o))])
timed("poisson512_stored_apply", lambda: m.apply_to_vector(xt))
timed("poisson512_stored_residual", lambda: m.residual_norm2(b, xt))
m.close()
m = handle(v, c, r, None, {"CCP_GS_STRUCTURED": "0", "CCP_GS_ONE_BLOCK": "0", "CCP_GS_PIPELINE": "0"})
solves(m, b, out, [("poisson512_per_group_20_no_rule", lambda m, b, o: m.gauss_seidel(b, 0.0, 20, check_every=0, ordering=LEX, out=o))])
m.close()
m = handle(v, c, r, None, {})
timed("poisson512_twin_apply", lambda: m.apply_to_vector(xt))
timed("poisson512_twin_residual", lambda: m.residual_norm2(b, xt))
m.close()

mask = synth.disc_mask(2048, 2048, seed=4321)
v, c, r, colour, ys, xs = synth.masked_laplacian_csr(mask)
n = len(ys)
xt = synth.x_true(n, 4321)
b = synth.csr_apply(v, c, r, xt)
out = np.empty(n)
m = handle(v, c, r, colour, {"CCP_GS_MASKED": "0"})
solves(m, b, out, [("mask2048_stored_colour_50_every_sweep", lambda m, b, o: m.gauss_seidel(b, 1e-300, 50, check_every=1, out=o)),
                   ("mask2048_stored_cg_fused_50", lambda m, b, o: m.conjugate_gradient(b, 1e-300, 50)),
                   ("mask2048_stored_cg_jacobi_50", lambda m, b, o: m.conjugate_gradient_jacobi(b, 1e-300, 50))])
timed("mask2048_stored_apply", lambda: m.apply_to_vector(xt))
timed("mask2048_stored_residual", lambda: m.residual_norm2(b, xt))
m.close()
m = handle(v, c, r, colour, {})
solves(m, b, out, [("mask2048_region_twin_50_every_sweep", lambda m, b, o: m.gauss_seidel(b, 1e-300, 50, check_every=1, out=o))])
assert m.last_path().startswith("region grid"), m.last_path()
timed("mask2048_region_twin_apply", lambda: m.apply_to_vector(xt))
timed("mask2048_region_twin_residual", lambda: m.residual_norm2(b, xt))
m.close()
