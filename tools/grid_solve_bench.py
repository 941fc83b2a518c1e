#!/usr/bin/env python3
"""The four grid solves whose host code NOTES §R22.1 touched, at a launch-bound shape (752x566x3) and at 4096^2 x3: Gauss-Seidel
with the rule after every sweep (256 sweeps) and CG (50 iterations), on one block and on a one-rank row block over real RCCL.
Per solve: median, min and max over 7 calls (after a warm one) of the call's own event time.  CCP_GS_LIB chooses the build;
alternate two builds in one command to compare them.  One JSON line per (shape, solve)."""
import json, os, statistics, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from coursecomputationalphotography_amd import capi

REPEAT = 7
comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
for W, H, C in ((752, 566, 3), (4096, 4096, 3)):
    g = capi.Grid(W, H, C)
    g.randomize_x(1234, 0.0, 255.0)
    g.b_from_x()

    def timed(fn, x0):
        ts = []
        for k in range(REPEAT + 1):
            g.fill_x(x0)
            reps = fn()
            if k:
                ts.append(sum(r.seconds for r in reps) if fn in (cg1, cgrb) else reps[0].seconds)
        return ts, reps[0].iterations

    gs1 = lambda: g.gauss_seidel(1e-300, 256, 1)
    gsrb = lambda: g.gauss_seidel_rowblocked(1e-300, 256, 1)
    cg1 = lambda: g.conjugate_gradient(1e-30, 50)
    cgrb = lambda: g.conjugate_gradient_rowblocked(1e-30, 50)
    for name, fn, x0, attach in (("gs_checked_one_block", gs1, 1.0, False), ("cg_one_block", cg1, 0.0, False),
                                 ("gs_checked_row_block", gsrb, 1.0, True), ("cg_row_block", cgrb, 0.0, True)):
        if attach:
            g.attach_comm(comm)
        ts, its = timed(fn, x0)
        if attach:
            g.attach_comm(None)
        print(json.dumps({"case": f"{W}x{H}x{C}", "solve": name, "iterations": its, "ms_median": 1e3 * statistics.median(ts),
                          "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts)}), flush=True)
    g.close()
comm.close()
