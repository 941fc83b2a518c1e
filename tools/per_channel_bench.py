#!/usr/bin/env python3
"""A stack of N single-channel WLS systems with DIFFERENT weights on one MI355X, three ways (include/ccp_gs.h, "One
operator per channel"):

  a  N one-channel weighted handles, solved one after another -- the only way before the per-channel operator;
  b  per-channel handles, sequential channels;
  c  per-channel handles, batched channels (k_pco_*: one PCG loop whose launches serve every channel of a handle).

A handle holds at most 8 channels, so the stack is spread over ceil(N / 8) per-channel handles (2 for the default N = 16),
solved one after another.  Every leg runs the rescaled hierarchy, nu = 2, to 1e-10 ||b_0|| from x = f, on the systems of
tensor_ops.wls_smooth: image i is a seeded patch image, its weights wls_weights(image i), lambda = 1.

Method.  The three legs alternate in ONE process; a leg's figure in an alternation is the best of 3 solves (host clock
around the solve calls, which end in a read-back; x is reset by re-assembling, outside the clock); at least 3
alternations; a leg's spread is (max - min) / min of its per-alternation figures -- the noise a difference between legs
has to exceed.  The hierarchies are built by one untimed solve per leg.  `launches_modelled` is NOT counted: it is a model
of the kernel launches the host loop issues for the solve, restated here from the loop's structure in csrc/ccp_grid_mg.hip
(set-up 5 + V, then 7 + V per issued iteration with V = 3 x (levels above the tail) + 1, iterations issued in batches of 16
until every channel of the loop has stopped), and goes stale if that loop changes.
The legs must agree bit for bit: the tool checks x of b and c against a and says so in `bits_equal`.

One JSON line per size and leg.

usage: per_channel_bench.py [--sizes 256x256,752x566] [--stack 16] [--alternations 3] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from coursecomputationalphotography_amd import capi, tensor_ops  # noqa: E402

MAX_C = 8
CAP = 1000
TAIL_SIDE = 32


def patch_image(W, H, seed):
    """Flat 16-px patches x 230 plus 25 x noise, one channel, u8 (tools/weighted_bench.py's image)."""
    rng = np.random.default_rng(seed)
    patches = rng.random((H // 16 + 1, W // 16 + 1))
    img = np.repeat(np.repeat(patches, 16, axis=0), 16, axis=1)[:H, :W] * 230.0
    return np.clip(img + 25.0 * rng.random((H, W)), 0, 255).astype(np.uint8)


def handle(W, H, C, channels):
    g = capi.Grid(W, H, C, weighted=True)
    g.mg_set_hierarchy("rescaled")
    g.mg_set_channels(channels)
    return g


def launches_modelled(levels, iterations):
    """A model (see the module text) of the kernel launches of one PCG loop whose slowest channel stops after `iterations`."""
    sides = [(d.shape[1], d.shape[0]) for d, _, _ in levels]
    tail = next((k for k in range(1, len(sides)) if sides[k][0] <= TAIL_SIDE and sides[k][1] <= TAIL_SIDE), len(sides))
    v = 3 * tail + 1 if len(sides) > 1 else 1
    issued = min(CAP, 16 * math.ceil((iterations + 1) / 16))
    return 5 + v + issued * (7 + v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256,752x566")
    ap.add_argument("--stack", type=int, default=16)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        N = a.stack
        imgs = [torch.from_numpy(patch_image(W, H, 100 + i)).to(dev) for i in range(N)]
        wts = [tensor_ops.wls_weights(im) for im in imgs]
        one = torch.ones(H, W, dtype=torch.float64, device=dev)
        # leg a: N one-channel handles
        singles = []
        for i in range(N):
            g = handle(W, H, 1, "sequential")
            g.set_weights_tensor(wts[i][0], wts[i][1], one)
            singles.append((g, imgs[i].unsqueeze(-1)))
        # legs b, c: per-channel handles of up to MAX_C channels
        stacks = {}
        for leg, mode in (("b", "sequential"), ("c", "batched")):
            stacks[leg] = []
            for lo in range(0, N, MAX_C):
                idx = list(range(lo, min(N, lo + MAX_C)))
                g = handle(W, H, len(idx), mode)
                g.set_weights_per_channel_tensor(torch.stack([wts[i][0] for i in idx], -1), torch.stack([wts[i][1] for i in idx], -1), one)
                stacks[leg].append((g, torch.stack([imgs[i] for i in idx], -1)))
        groups = {"a": singles, "b": stacks["b"], "c": stacks["c"]}
        singles[0][0].assemble_weighted_rhs_tensor(None, None, singles[0][1], init_x=True)
        eps = 1e-10 * float(np.linalg.norm(singles[0][0].get_b(0)))

        def run(leg):
            """One solve of the whole stack: (seconds, iterations per image)."""
            for g, f in groups[leg]:
                g.assemble_weighted_rhs_tensor(None, None, f, init_x=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            reps = [g.mg_conjugate_gradient(eps, CAP, 2) for g, _ in groups[leg]]
            dt = time.perf_counter() - t0
            its = [int(r.iterations) for rs in reps for r in rs]
            assert all(r.converged for rs in reps for r in rs), (leg, its)
            return dt, its

        def solution(leg):
            return [g.get_x(c) for g, _ in groups[leg] for c in range(g.C)]

        its, xs = {}, {}
        for leg in "abc":                                            # untimed: builds the hierarchies and the work sets
            _, its[leg] = run(leg)
            xs[leg] = solution(leg)
        equal = {leg: all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(xs[leg], xs["a"])) and its[leg] == its["a"]
                 for leg in "bc"}
        best = {leg: [] for leg in "abc"}
        for _ in range(max(3, a.alternations)):
            for leg in "abc":
                best[leg].append(min(run(leg)[0] for _ in range(3)))
        levels = singles[0][0].mg_levels()
        for leg in "abc":
            t = best[leg]
            if leg == "c":
                n_launch = sum(launches_modelled(levels, max(its[leg][lo:lo + MAX_C])) for lo in range(0, N, MAX_C))
            else:
                n_launch = sum(launches_modelled(levels, i) for i in its[leg])
            lines.append(dict(tool="per_channel_bench", size=f"{W}x{H}", stack=N, leg=leg, handles=len(groups[leg]),
                              ms_best=1e3 * min(t), ms_median=1e3 * float(np.median(t)), spread=(max(t) - min(t)) / min(t),
                              ms_per_alternation=[1e3 * v for v in t], iterations=its[leg], launches_modelled=n_launch,
                              bits_equal=True if leg == "a" else equal[leg], epsilon=eps))
            print(json.dumps(lines[-1]), flush=True)
        for grp in groups.values():
            for g, _ in grp:
                g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
