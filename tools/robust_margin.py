#!/usr/bin/env python3
"""How far an inner solve that stops at a relative residual may move the energy of the robust IRLS loop: the figure behind
E_MARGIN of tests/test_gpu_robust_irls.py, by NOTES R38.1's method.  CPU only (numpy): on the outlier image of
tests/robust_helpers.py the dense loop with exact solves (np.linalg.solve) against the same loop with every solve moved
along a seeded random direction to the relative residual --tolerance, --seeds seeds; reported per case: the largest
|E - E'| at any step and the largest step-to-step change of E from the second step on, for either loop.  One JSON line per
case, appended to --out."""
import argparse, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "tests")))
import numpy as np
import robust_helpers as bh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--tolerance", type=float, default=1e-10)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r39_robust_margin.jsonl"))
    a = ap.parse_args()
    clean, noisy = bh.outlier_image(a.width, a.height)
    for coupling, dp, per_channel in bh.CASES:
        run = lambda **kw: bh.dense_irls_robust(noisy, None, None, "charbonnier", coupling, bh.STRENGTH, bh.EPS, dp, bh.DATA_SCALE, bh.DATA_EPS,
                                                bh.OUTER, per_channel, **kw)
        its, exact, _ = run()
        gap, rise = 0.0, float(np.diff(exact[2:]).max())
        for seed in range(a.seeds):
            _, moved, _ = run(perturb=a.tolerance, seed=seed)
            gap = max(gap, float(np.abs(np.array(moved) - np.array(exact)).max()))
            rise = max(rise, float(np.diff(moved[2:]).max()))
        row = {"canvas": f"{a.width}x{a.height}x2", "coupling": coupling, "data_penalty": dp, "per_channel": per_channel,
               "tolerance": a.tolerance, "seeds": a.seeds, "largest_energy_gap": gap, "largest_step_to_step_change_from_step_1": rise,
               "energy": exact, "rmse_input": bh.rmse(noisy, clean), "rmse_result": bh.rmse(its[-1], clean)}
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
