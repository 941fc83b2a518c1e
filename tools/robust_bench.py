#!/usr/bin/env python3
"""Reweighting the edges AND lambda of an installed operator from the solution, on one MI355X: tools/reweight_bench.py's
protocol to the letter -- a weighted handle with random fp64 base weights in [0.5, 2), lambda = 1e-2, the rescaled
hierarchy, fp64, sequential channels, the point smoother, charbonnier / pixel, at 752x566x3 and 4096^2 x3, x a random
image in [0, 255], random float32 guidance -- and a random fp64 f in [0, 255] for the data term.

Four legs, each the wall time (time.perf_counter) of giving the handle the next operator, ending with the stream idle:
  (a) robust_q   reweight_robust_tensor with a QUADRATIC data term of scale 1: the marching kernel doing the older call's work
  (b) reweight   reweight_tensor on the same inputs: the thread-per-pixel kernel
  (c) robust     reweight_robust_tensor with a Charbonnier data term
  (d) torch      the route to (c) a caller had before: get_x_tensor, lambda by torch element-wise ops in the header's
                 operation order, reweight_tensor(lam=that plane)
The legs alternate between two values of `scale`, so no call finds the values it left.  One untimed run of each leg, then
--rounds alternations in one process; in each, every leg runs three times and its best counts.  Per leg the best of all, the
per-alternation bests and their spread (max / min: the noise floor the ratios are read against) are reported.  Before the
timing (a)'s weights are asserted equal to (b)'s and (c)'s weights and lambda to (d)'s, bit for bit; after it the handles the
pairs leave are compared (level 1 of the hierarchy).  One JSON line per case, appended to --out.

The rows per strip of the marching kernel are the library's (CCP_GS_ROBUST_ROWS=4|8|16|32 overrides them for a process: run
the tool once per value to choose); the line records what the process ran with.

Not measured here: f32 precision, batched channels, the line smoother, one operator per channel, fixed pixels, the other
penalties, EDGE coupling."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS, EPSILON, SCALES = 1e-2, 2, 1e-2, (0.75, 1.5)
DATA_SCALE, DATA_EPSILON = 1.0, 5e-2


def torch_lambda(x, f, base, scale, eps):
    """the header's Charbonnier lambda in torch ops: one element-wise kernel per operation, the channels accumulated in order"""
    acc = torch.zeros_like(base)
    for c in range(x.shape[2]):
        r = f[:, :, c] - x[:, :, c]
        acc = acc + r * r
    one = torch.ones((), dtype=torch.float64, device=x.device)
    return base * (scale * (one / torch.sqrt(acc + eps * eps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r39_robust_bench.jsonl"))
    a = ap.parse_args()
    penalty, coupling = "charbonnier", "pixel"
    if not torch.cuda.is_available():
        sys.exit("robust_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        bwx, bwy = ((0.5 + 1.5 * torch.rand(H, W, generator=gen, dtype=torch.float64)).to(dev) for _ in range(2))
        gx, gy = (torch.randn(H, W, Cn, generator=gen, dtype=torch.float32).to(dev) for _ in range(2))
        f = (255.0 * torch.rand(H, W, Cn, generator=gen, dtype=torch.float64)).to(dev)
        lam = torch.full((), LAMBDA, dtype=torch.float64, device=dev).expand(H, W)
        g = capi.Grid(W, H, Cn, device=0, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights_tensor(bwx, bwy, lam)
        g.mg_prepare(SWEEPS)
        g.randomize_x(11, 0.0, 255.0)
        turn = [0]
        edges = dict(gx=gx, gy=gy, base_wx=bwx, base_wy=bwy)

        def next_scale():
            turn[0] ^= 1
            return SCALES[turn[0]]

        def leg_robust_q(**out):
            g.reweight_robust_tensor(penalty, coupling, next_scale(), EPSILON, "quadratic", 1.0, None, lam=lam, **edges, **out)

        def leg_reweight(**out):
            g.reweight_tensor(penalty, coupling, next_scale(), EPSILON, lam=lam, **edges, **out)

        def leg_robust(**out):
            g.reweight_robust_tensor(penalty, coupling, next_scale(), EPSILON, "charbonnier", DATA_SCALE, DATA_EPSILON, f=f, lam=lam, **edges, **out)

        def leg_torch(**out):
            formed = torch_lambda(g.get_x_tensor(), f, lam, DATA_SCALE, DATA_EPSILON)
            g.reweight_tensor(penalty, coupling, next_scale(), EPSILON, lam=formed, **edges, **out)
            return formed

        # (a) against (b) and (c) against (d), to the bit, for both scales
        same = lambda p, q: torch.equal(p.view(torch.int64), q.view(torch.int64))
        o = [torch.empty(H, W, dtype=torch.float64, device=dev) for _ in range(5)]
        for _ in SCALES:
            leg_robust_q(out_wx=o[0], out_wy=o[1], out_lambda=o[2])
            turn[0] ^= 1
            leg_reweight(out_wx=o[3], out_wy=o[4])
            torch.cuda.synchronize()
            assert same(o[0], o[3]) and same(o[1], o[4]) and same(o[2], lam.contiguous()), "(a) differs from (b)"
            turn[0] ^= 1
            leg_robust(out_wx=o[0], out_wy=o[1], out_lambda=o[2])
            turn[0] ^= 1
            formed = leg_torch(out_wx=o[3], out_wy=o[4])
            torch.cuda.synchronize()
            assert same(o[0], o[3]) and same(o[1], o[4]) and same(o[2], formed), "(c) differs from (d)"
        status = g.operator_status()
        del o, formed
        legs = {"robust_q": leg_robust_q, "reweight": leg_reweight, "robust": leg_robust, "torch": leg_torch}

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
        # the handles the pairs leave, on the same scale
        level1 = []
        for mine, theirs in ((leg_robust_q, leg_reweight), (leg_robust, leg_torch)):
            turn[0] = 0
            mine()
            left = [p.copy() for p in g.mg_level(1)]
            turn[0] = 0
            theirs()
            level1.append(all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(left, g.mg_level(1))))
        g.close()
        assert all(level1), "the handles differ at level 1"
        rows = os.environ.get("CCP_GS_ROBUST_ROWS", "library default")
        row = {"case": name, "penalty": penalty, "coupling": coupling, "rows_per_strip": rows, "operator_status": status,
               "a_equals_b_and_c_equals_d_to_the_bit": True, "level1_equal": level1}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
            row[f"{k}_spread"] = max(v) / min(v)
        row["a_over_b"] = row["robust_q_ms_best"] / row["reweight_ms_best"]
        row["c_over_d"] = row["robust_ms_best"] / row["torch_ms_best"]
        row["c_over_a"] = row["robust_ms_best"] / row["robust_q_ms_best"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
