#!/usr/bin/env python3
"""The null-space mode of weighted grid handles (CCP_MG_NULLSPACE_CONSTANT) on one MI355X: MG-PCG iterations and
milliseconds to 1e-10 |b| on a floating system (wx = wy = 1, or --weights random: uniform in [0.1, 10); lambda = 0, no
fixed pixel), in CONSTANT mode and, on the SAME consistent system, in NONE mode -- the only system on which the two can
be timed against each other: b = A x of a random x sums to zero up to rounding, and the loop without the projection
reaches 1e-10 |b| on it before its drift along the constants shows (on any other b it does not converge: NOTES R28.1).
--nullspace: a comma list of none / constant, alternated on the same handle, so none,constant,none,constant,none,constant
gives three alternations and `none` against itself as the noise floor.  --hierarchy, --precision, --smoother, --sweeps as
tools/weighted_bench.py.  One JSON line per case and run.  ms_per_pcg_iteration divides by the updates summed over the
channels; the CONSTANT figure includes the once-per-solve means and the closing shift (they lie inside the timed region)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"floating_16384sq": (16384, 16384, 1), "floating_4096sq_x3": (4096, 4096, 3), "floating_752x566_x3": (752, 566, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--nullspace", default="none,constant", help="comma list of none / constant, in the order to run them")
    ap.add_argument("--hierarchy", default="galerkin", help="comma list of galerkin / rescaled")
    ap.add_argument("--precision", default="f64", help="comma list of f64 / f32")
    ap.add_argument("--smoother", default="point", help="comma list of point / line")
    ap.add_argument("--weights", default="unit", choices=["unit", "random"])
    ap.add_argument("--sweeps", type=int, default=0, help="0: the smoother's default, 2 point sweeps or 1 line sweep")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=50)
    a = ap.parse_args()
    lists = {}
    for flag, table in (("nullspace", capi.MG_NULLSPACES), ("hierarchy", capi.MG_HIERARCHIES), ("precision", capi.MG_PRECISIONS),
                        ("smoother", capi.MG_SMOOTHERS)):
        lists[flag] = getattr(a, flag).split(",")
        for v in lists[flag]:
            if v not in table:
                ap.error(f"--{flag}: {v!r} is not one of {sorted(table)}")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, C = CASES[name]
        g = capi.Grid(W, H, C, weighted=True)
        if a.weights == "random":
            gen = torch.Generator(device=dev).manual_seed(7)
            wx, wy = (0.1 + 9.9 * torch.rand((H, W), generator=gen, device=dev, dtype=torch.float64) for _ in range(2))
            g.set_weights_tensor(wx, wy, None)
        else:
            g.set_weights_tensor(None, None, None)
        g.randomize_x(1234, 0.0, 255.0)
        g.b_from_x()                                                # consistent: b = A x
        g.synchronize()
        runs = [(sm, p, h, ns) for sm in lists["smoother"] for p in lists["precision"] for h in lists["hierarchy"] for ns in lists["nullspace"]]
        for run, (smoother, precision, hierarchy, nullspace) in enumerate(runs):
            g.mg_set_smoother(smoother)
            g.mg_set_hierarchy(hierarchy)
            g.mg_set_precision(precision)
            g.mg_set_nullspace(nullspace)
            best = None
            for k in range(a.repeat + 1):                           # the first solve of a mode builds what it needs: not timed
                g.fill_x(0.0)
                _, bb = g.residual_norm2()
                eps = 1e-10 * float(np.sqrt(bb.max()))
                reps = g.mg_conjugate_gradient(eps, a.max_iterations, a.sweeps)
                secs = sum(r.seconds for r in reps)
                if k and (best is None or secs < best[0]):
                    best = (secs, [r.iterations for r in reps], [bool(r.converged) for r in reps])
            rr, bb = g.residual_norm2()
            secs, its, conv = best
            updates = sum(i + 1 for i in its)
            print(json.dumps({"case": name, "width": W, "height": H, "channels": C, "weights": a.weights, "nullspace": nullspace,
                              "hierarchy": hierarchy, "precision": precision, "smoother": smoother, "run": run,
                              "smoothing_sweeps": a.sweeps or (1 if smoother == "line" else 2), "max_iterations": a.max_iterations,
                              "iterations": its, "converged": conv, "ms_to_1e-10": secs * 1e3, "ms_per_pcg_iteration": secs * 1e3 / updates,
                              "rel_residual": float(np.sqrt(rr / bb).max())}), flush=True)
        g.close()


if __name__ == "__main__":
    main()
