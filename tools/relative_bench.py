#!/usr/bin/env python3
"""The enqueue-only multigrid PCG with its stop test relative to |b| (ccp_grid_mg_conjugate_gradient_enqueue_relative)
against the absolute enqueue call on one MI355X, by tools/enqueue_bench.py's protocol: a weighted handle with unit weights,
lambda = 1e-2, the rescaled hierarchy, fp64, the point smoother, at 752x566x3 and 4096^2 x3.  The system is manufactured
(b = A x*, x* uniform [0, 255)) and channel 0's right-hand side is given to every channel, so one threshold serves all
of them; every timed solve starts from x = 0.

Two legs, each the wall time of one solve until the stream is idle (time.perf_counter around it):
  (a) absolute  fill x = 0 + mg_conjugate_gradient_enqueue at epsilon = the eps a prior relative solve reported
  (b) relative  fill x = 0 + mg_conjugate_gradient_enqueue_relative(0, epsilon_rel)
max_iteration is the count that prior solve needed plus the one update that passes the threshold.  Both legs must report
the same iterations, or the comparison is void (the tool exits).  One untimed run of every leg, then the legs alternated
--rounds times in one process; per leg the best and all the times are reported, (b)/(a), and (a)'s own spread
(worst / best) as the noise floor.  One JSON line per case, appended to --out."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from coursecomputationalphotography_amd import capi

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS, REL = 1e-2, 2, 1e-10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r34_relative_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relative_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        one = torch.ones((), dtype=torch.float64, device=dev).expand(H, W)
        lam = torch.full((), LAMBDA, dtype=torch.float64, device=dev).expand(H, W)
        g = capi.Grid(W, H, Cn, device=0, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights_tensor(one, one, lam)
        g.randomize_x(1, 0.0, 255.0)
        g.b_from_x()
        b0 = g.get_b(0)
        for c in range(1, Cn):                                  # identical channels: one threshold serves all
            g.set_b(b0, c)
        g.mg_prepare(SWEEPS)
        rel_report = torch.zeros((Cn, 8), dtype=torch.float64, device=dev)
        abs_report = torch.zeros((Cn, 6), dtype=torch.float64, device=dev)
        g.fill_x(0.0)
        g.mg_conjugate_gradient_enqueue_relative(0.0, REL, 200, SWEEPS, rel_report)
        torch.cuda.synchronize()
        first = rel_report.cpu()
        assert bool((first[:, 1] == 1.0).all()), first
        assert bool((first[:, 7] == first[0, 7]).all()), first
        eps = float(first[0, 7])
        cap = int(first[:, 0].max()) + 1

        def leg_absolute():
            g.fill_x(0.0)
            g.mg_conjugate_gradient_enqueue(eps, cap, SWEEPS, abs_report)

        def leg_relative():
            g.fill_x(0.0)
            g.mg_conjugate_gradient_enqueue_relative(0.0, REL, cap, SWEEPS, rel_report)

        legs = {"absolute": leg_absolute, "relative": leg_relative}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        x = {}
        for k, fn in legs.items():                               # one untimed run of every leg
            timed(fn)
            x[k] = g.get_x_tensor().clone()
        its = {"absolute": abs_report[:, 0].tolist(), "relative": rel_report[:, 0].tolist()}
        conv = {"absolute": abs_report[:, 1].tolist(), "relative": rel_report[:, 1].tolist()}
        if its["absolute"] != its["relative"] or conv["absolute"] != conv["relative"]:
            sys.exit(f"relative_bench: {name}: the legs ran different solves ({its}, {conv}): the comparison is void")
        same = bool(torch.equal(x["absolute"].view(torch.int64), x["relative"].view(torch.int64)))
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        row = {"case": name, "max_iteration": cap, "iterations": its["relative"], "converged": conv["relative"], "epsilon_rel": REL,
               "epsilon": eps, "bnorm": float(first[0, 6]), "relative_x_equals_absolute_bits": same}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
        row["relative_over_absolute"] = row["relative_ms_best"] / row["absolute_ms_best"]
        row["absolute_spread"] = max(times["absolute"]) / min(times["absolute"])
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        g.close()


if __name__ == "__main__":
    main()
