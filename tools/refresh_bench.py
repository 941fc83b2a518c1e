#!/usr/bin/env python3
"""New weights on an installed operator, two ways, on one MI355X: a weighted handle with random fp64 weights in [0.5, 2),
lambda = 1e-2, the rescaled hierarchy, fp64, sequential channels, the point smoother, at 752x566x3 (the reference's own
image size) and 4096^2 x3.

Two legs, each the wall time (time.perf_counter) of giving the handle the next set of weights, ending with the stream idle:
  (a) set      set_weights_tensor + mg_prepare: the setter validates and reads its verdict back, drops the hierarchy, and
               prepare rebuilds and reallocates everything
  (b) refresh  refresh_weights_tensor + torch.cuda.synchronize: enqueue only, nothing allocated
The two legs install the same weights alternately (two sets, swapped every time, so no call finds the values it left).  One
untimed run of each leg, then the legs alternated --rounds times in one process; per leg the best and all the times are
reported, and (a)'s own spread is the noise floor.  After the timing the refreshed handle is checked against a fresh one:
level 1 of both hierarchies equal as bits.  One JSON line per case, appended to --out.

Not measured here: f32 precision, batched channels, the line smoother, one operator per channel, fixed pixels, and a training
loop around the refresh."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS = 1e-2, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r32_refresh_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refresh_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        sets = [[(0.5 + 1.5 * torch.rand(H, W, generator=gen, dtype=torch.float64)).to(dev) for _ in range(2)] for _ in range(2)]
        lam = torch.full((), LAMBDA, dtype=torch.float64, device=dev).expand(H, W)
        g = capi.Grid(W, H, Cn, device=0, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights_tensor(sets[0][0], sets[0][1], lam)
        g.mg_prepare(SWEEPS)
        turn = [0]

        def next_weights():
            turn[0] ^= 1
            return sets[turn[0]]

        def leg_set():
            wx, wy = next_weights()
            g.set_weights_tensor(wx, wy, lam)
            g.mg_prepare(SWEEPS)

        def leg_refresh():
            wx, wy = next_weights()
            g.refresh_weights_tensor(wx, wy, lam)

        legs = {"set": leg_set, "refresh": leg_refresh}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for fn in legs.values():                             # one untimed run of every leg
            timed(fn)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        # the handle's last operator change was a refresh: its level 1 against a fresh handle's
        wx, wy = sets[turn[0]]
        status = g.operator_status()
        fresh = capi.Grid(W, H, Cn, device=0, weighted=True)
        fresh.mg_set_hierarchy("rescaled")
        fresh.set_weights_tensor(wx, wy, lam)
        same = all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(g.mg_level(1), fresh.mg_level(1)))
        fresh.close()
        row = {"case": name, "operator_status": status, "refreshed_level1_equals_fresh_bits": bool(same)}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
        row["refresh_over_set"] = row["refresh_ms_best"] / row["set_ms_best"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        g.close()


if __name__ == "__main__":
    main()
