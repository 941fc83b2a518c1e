#!/usr/bin/env python3
"""A new set of fixed pixels on an installed operator, three ways, on one MI355X: tools/refresh_bench.py's protocol -- a
weighted handle with random fp64 weights in [0.5, 2), lambda = 1e-2, the rescaled hierarchy, fp64, sequential channels, the
point smoother, at 752x566x3 and 4096^2 x3 -- on a handle that reserves its constraint planes, with two masks: everything
outside a centred ellipse fixed, and sparse anchors [8::16, 8::16].

Three legs, each the wall time (time.perf_counter) of giving the handle the next weights, ending with the stream idle:
  (a) refresh_constrained  refresh_constrained_tensor + torch.cuda.synchronize: weights and mask, enqueue only
  (b) refresh_weights      refresh_weights_tensor + torch.cuda.synchronize: weights alone, the mask kept
  (c) set                  set_weights_tensor with the mask + mg_prepare: validation read back, hierarchy rebuilt
Legs (a) and (c) alternate between two masks of the kind (the second is the first shifted by three pixels) and all legs
between two sets of weights, so no call finds the values it left.  One untimed run of each leg, then the legs alternated
--rounds times in one process; per leg the best and all the times are reported.  a/c is the gain, a/b the cost of carrying
the mask; (c)'s and (b)'s own spread over the alternation (max / min) is the noise floor they are read against.  After the
timing the refreshed handle is checked against a fresh one (level 1 of both hierarchies and the three counts equal).
`--memory`: also the device memory a reserved and an unreserved handle of the case take (torch.cuda.mem_get_info around
their creation, setter and prepare), beside the model of 24 bytes per pixel and set.  One JSON line per case and mask,
appended to --out.

Not measured here: f32 precision, batched channels, the line smoother, one operator per channel, and a training loop around
the refresh."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS = 1e-2, 2


def masks(kind, W, H, dev):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = []
    for shift in (0, 3):
        if kind == "ellipse":
            m = (((x - shift - (W - 1) / 2) / (0.4 * W)) ** 2 + ((y - (H - 1) / 2) / (0.4 * H)) ** 2) > 1.0
        else:
            m = torch.zeros(H, W, dtype=torch.bool)
            m[8 + shift::16, 8 + shift::16] = True
        out.append(m.to(torch.uint8).to(dev))
    return out


def footprint(W, H, Cn, wx, wy, lam, fixed, reserve):
    """device bytes a handle takes from creation to prepared"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    g = capi.Grid(W, H, Cn, device=0, weighted=True)
    g.mg_set_hierarchy("rescaled")
    if reserve:
        g.reserve_constraints()
    g.set_weights_tensor(wx, wy, lam, fixed=fixed)
    g.mg_prepare(SWEEPS)
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info(0)[0]
    g.close()
    return used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--masks", default="ellipse,anchors")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r36_refresh_mask_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refresh_mask_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        sets = [[(0.5 + 1.5 * torch.rand(H, W, generator=gen, dtype=torch.float64)).to(dev) for _ in range(2)] for _ in range(2)]
        lam = torch.full((), LAMBDA, dtype=torch.float64, device=dev).expand(H, W)
        for kind in a.masks.split(","):
            fixed = masks(kind, W, H, dev)
            g = capi.Grid(W, H, Cn, device=0, weighted=True)
            g.mg_set_hierarchy("rescaled")
            g.reserve_constraints()
            g.set_weights_tensor(sets[0][0], sets[0][1], lam, fixed=fixed[0])
            g.mg_prepare(SWEEPS)
            turn, mturn = [0], [0]

            def next_weights():
                turn[0] ^= 1
                return sets[turn[0]]

            def next_mask():
                mturn[0] ^= 1
                return fixed[mturn[0]]

            def leg_constrained():
                wx, wy = next_weights()
                g.refresh_constrained_tensor(wx, wy, lam, next_mask())

            def leg_weights():
                wx, wy = next_weights()
                g.refresh_weights_tensor(wx, wy, lam)

            def leg_set():
                wx, wy = next_weights()
                g.set_weights_tensor(wx, wy, lam, fixed=next_mask())
                g.mg_prepare(SWEEPS)

            legs = {"refresh_constrained": leg_constrained, "refresh_weights": leg_weights, "set": leg_set}

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for fn in legs.values():                         # one untimed run of every leg
                timed(fn)
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    times[k].append(timed(fn))
            leg_constrained()                                # the last change is a constrained refresh: against a fresh handle
            wx, wy = sets[turn[0]]
            status = g.operator_status()
            fresh = capi.Grid(W, H, Cn, device=0, weighted=True)
            fresh.mg_set_hierarchy("rescaled")
            fresh.set_weights_tensor(wx, wy, lam, fixed=fixed[mturn[0]])
            same = all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(g.mg_level(1), fresh.mg_level(1)))
            same = same and g.constraint_info() == fresh.constraint_info()
            counts = g.constraint_info()
            fresh.close()
            g.close()
            row = {"case": name, "mask": kind, "fixed_pixels": counts[0], "boundary_edges": counts[2], "operator_status": status,
                   "refreshed_level1_and_counts_equal_fresh": bool(same)}
            for k, v in times.items():
                row[f"{k}_ms_best"] = min(v)
                row[f"{k}_ms_all"] = v
            row["a_over_c"] = row["refresh_constrained_ms_best"] / row["set_ms_best"]
            row["a_over_b"] = row["refresh_constrained_ms_best"] / row["refresh_weights_ms_best"]
            row["c_spread"] = max(times["set"]) / min(times["set"])
            row["b_spread"] = max(times["refresh_weights"]) / min(times["refresh_weights"])
            if a.memory:
                row["bytes_reserved"] = footprint(W, H, Cn, sets[0][0], sets[0][1], lam, None, True)
                row["bytes_unreserved"] = footprint(W, H, Cn, sets[0][0], sets[0][1], lam, None, False)
                row["bytes_model_24_per_pixel"] = 24 * W * H
            line = json.dumps(row)
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
