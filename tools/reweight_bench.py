#!/usr/bin/env python3
"""Reweighting an installed operator from the solution, three ways, on one MI355X: tools/refresh_bench.py's protocol -- a
weighted handle with random fp64 base weights in [0.5, 2), lambda = 1e-2, the rescaled hierarchy, fp64, sequential channels,
the point smoother, at 752x566x3 and 4096^2 x3 -- with x a random image in [0, 255] and random float32 guidance.

Three legs, each the wall time (time.perf_counter) of giving the handle the next weights, ending with the stream idle:
  (a) reweight   reweight_tensor from the handle's x: one fused pass forms the weights in registers, then the refresh's launches
  (b) torch      the route a caller has without it: get_x_tensor, the same weights by torch element-wise ops in the header's
                 operation order, refresh_weights_tensor
  (c) refresh    refresh_weights_tensor alone on two ready fp64 planes: what is left when the weights cost nothing
The legs alternate between two values of `scale`, so no call finds the values it left.  One untimed run of each leg, then
--rounds alternations in one process; in each, every leg runs three times and its best counts.  Per leg the best of all and
the per-alternation bests are reported; a/b is the gain over the torch route, a/c the cost of forming the weights, and every
leg's own spread over the alternations (max / min) is the noise floor the ratios are read against.  Before the timing the
weights of (a) (its out_wx / out_wy) are asserted equal to the bit to those of (b), and after it the handle (a) leaves is
checked against the one (b) leaves (level 1 of both hierarchies).  One JSON line per case, appended to --out.

The byte model, per pixel with C channels: (a) reads 8C (x) + 8C (gx, gy) and writes 32 (d, we, ws, lambda); (b) adds the
16C of get_x (read and write), the element-wise passes and 32 for writing and re-reading the two planes.

Not measured here: f32 precision, batched channels, the line smoother, one operator per channel, fixed pixels."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS, EPSILON, SCALES = 1e-2, 2, 1e-2, (0.75, 1.5)


def torch_weights(x, gx, gy, bwx, bwy, penalty, coupling, scale, eps):
    """the header's definition in torch ops: one element-wise kernel per operation, the channels accumulated in order"""
    H, W, Cn = x.shape
    qx, qy = torch.zeros_like(bwx), torch.zeros_like(bwy)
    ax, ay = torch.zeros_like(bwx[:, :-1]), torch.zeros_like(bwy[:-1])
    for c in range(Cn):
        r = gx[:, :-1, c].to(torch.float64) - (x[:, 1:, c] - x[:, :-1, c])
        ax = ax + r * r
        r = gy[:-1, :, c].to(torch.float64) - (x[1:, :, c] - x[:-1, :, c])
        ay = ay + r * r
    qx[:, :-1], qy[:-1] = ax, ay
    if coupling == "pixel":
        qx = qy = qx + qy

    def phi(q):
        one = torch.ones((), dtype=torch.float64, device=q.device)
        if penalty == "charbonnier":
            return one / torch.sqrt(q + eps * eps)
        if penalty == "huber":
            return one / torch.clamp_min(torch.sqrt(q), eps)
        return one / (torch.sqrt(q) + eps)

    wx, wy = bwx * (scale * phi(qx)), bwy * (scale * phi(qy))
    wx[:, -1] = 0.0
    wy[-1] = 0.0
    return wx, wy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--penalty", default="charbonnier")
    ap.add_argument("--coupling", default="pixel")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r38_reweight_bench.jsonl"))
    a = ap.parse_args()
    capi.reweight_ids(a.penalty, a.coupling)
    if not torch.cuda.is_available():
        sys.exit("reweight_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        bwx, bwy = ((0.5 + 1.5 * torch.rand(H, W, generator=gen, dtype=torch.float64)).to(dev) for _ in range(2))
        gx, gy = (torch.randn(H, W, Cn, generator=gen, dtype=torch.float32).to(dev) for _ in range(2))
        lam = torch.full((), LAMBDA, dtype=torch.float64, device=dev).expand(H, W)
        g = capi.Grid(W, H, Cn, device=0, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights_tensor(bwx, bwy, lam)
        g.mg_prepare(SWEEPS)
        g.randomize_x(11, 0.0, 255.0)
        turn = [0]

        def next_scale():
            turn[0] ^= 1
            return SCALES[turn[0]]

        def leg_reweight():
            g.reweight_tensor(a.penalty, a.coupling, next_scale(), EPSILON, gx=gx, gy=gy, base_wx=bwx, base_wy=bwy, lam=lam)

        def leg_torch():
            wx, wy = torch_weights(g.get_x_tensor(), gx, gy, bwx, bwy, a.penalty, a.coupling, next_scale(), EPSILON)
            g.refresh_weights_tensor(wx, wy, lam)

        ready = [torch_weights(g.get_x_tensor(), gx, gy, bwx, bwy, a.penalty, a.coupling, s, EPSILON) for s in SCALES]

        def leg_refresh():
            next_scale()
            g.refresh_weights_tensor(ready[turn[0]][0], ready[turn[0]][1], lam)

        # the weights of (a) against those of (b), to the bit, for both scales
        owx, owy = (torch.empty(H, W, dtype=torch.float64, device=dev) for _ in range(2))
        equal = True
        for k, s in enumerate(SCALES):
            g.reweight_tensor(a.penalty, a.coupling, s, EPSILON, gx=gx, gy=gy, base_wx=bwx, base_wy=bwy, lam=lam, out_wx=owx, out_wy=owy)
            torch.cuda.synchronize()
            equal = equal and torch.equal(owx.view(torch.int64), ready[k][0].view(torch.int64))
            equal = equal and torch.equal(owy.view(torch.int64), ready[k][1].view(torch.int64))
        assert equal, "reweight_tensor's weights differ from the torch route's"
        status = g.operator_status()
        legs = {"reweight": leg_reweight, "torch": leg_torch, "refresh": leg_refresh}

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
                times[k].append(min(timed(fn) for _ in range(3)))
        # the handle (a) leaves against the one (b) leaves, on the same scale
        turn[0] = 0
        leg_reweight()
        mine = [p.copy() for p in g.mg_level(1)]
        turn[0] = 0
        leg_torch()
        same = all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(mine, g.mg_level(1)))
        g.close()
        row = {"case": name, "penalty": a.penalty, "coupling": a.coupling, "operator_status": status, "weights_equal_to_the_bit": bool(equal),
               "level1_equal": bool(same), "bytes_per_pixel_model_a": 16 * Cn + 32, "bytes_per_pixel_model_b_at_least": 32 * Cn + 64}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
            row[f"{k}_spread"] = max(v) / min(v)
        row["a_over_b"] = row["reweight_ms_best"] / row["torch_ms_best"]
        row["a_over_c"] = row["reweight_ms_best"] / row["refresh_ms_best"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
