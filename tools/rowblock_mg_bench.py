#!/usr/bin/env python3
"""ccp_grid_mg_conjugate_gradient_rowblocked on one rank of a real-RCCL communicator against the one-block
ccp_grid_mg_conjugate_gradient on the same handle: ms to 1e-10 |b|, iterations, and their ratio.  The row-blocked call
adds three one-double all-reduces per PCG iteration and a copy of x per channel and solve.  Best of --repeat solves
each; one JSON line per case (16384^2, 4096^2 x 3).  --out appends the lines to a file as well."""
import argparse, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
from coursecomputationalphotography_amd import capi

CASES = {"16384sq": (16384, 16384, 1), "4096sq_x3": (4096, 4096, 3)}

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default=",".join(CASES))
ap.add_argument("--sweeps", type=int, default=2)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
for name in a.cases.split(","):
    W, H, C = CASES[name]
    g = capi.Grid(W, H, C, 0, H, 1, 0)
    g.randomize_x(1234, 0.0, 255.0)
    g.b_from_x()
    _, bb = g.residual_norm2()
    eps = 1e-10 * float(np.sqrt(bb.max()))
    best = {}
    for _ in range(a.repeat):
        # alternate the two calls; each (re)attach or detach drops the other's hierarchy, so warm both up first
        for which in ("one_block", "rowblocked"):
            if which == "rowblocked":
                g.attach_comm(comm)
            for warm in (True, False):
                g.fill_x(0.0)
                reps = (g.mg_conjugate_gradient_rowblocked if which == "rowblocked" else g.mg_conjugate_gradient)(eps, 50, a.sweeps)
                if warm:
                    continue
                secs = sum(r.seconds for r in reps)
                if which not in best or secs < best[which][0]:
                    best[which] = (secs, [r.iterations for r in reps], [bool(r.converged) for r in reps])
            if which == "rowblocked":
                g.attach_comm(None)
    (t1, it1, c1), (tr, itr, cr) = best["one_block"], best["rowblocked"]
    line = {"case": name, "width": W, "height": H, "channels": C, "world": 1, "smoothing_sweeps": a.sweeps,
            "rccl_version": comm.info()["rccl_version"], "one_block_ms": t1 * 1e3, "one_block_iterations": it1,
            "rowblocked_ms": tr * 1e3, "rowblocked_iterations": itr, "converged": c1 + cr, "ratio": tr / t1}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    g.close()
comm.close()
