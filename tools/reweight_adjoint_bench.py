#!/usr/bin/env python3
"""The adjoint of the reweight pass against what a caller has without it, on one MI355X: tools/reweight_bench.py's protocol
-- random fp64 base weights in [0.5, 2), a random image in [0, 255], random float32 guidance, a shared f64 operator,
charbonnier / pixel, at 752x566x3 and 4096^2 x3; wall time (time.perf_counter) of each leg ending with the stream idle, one
untimed run of each, then --rounds alternations in which every leg runs three times and its best counts.

Legs:
  (a) adjoint    reweight_adjoint_tensor with every edge output (u, gx, gy, base_wx, base_wy) into ready tensors: one launch
  (b) autograd   torch.autograd.grad through a torch restatement of the same weights (the header's operation order, one
                 element-wise kernel per operation), the forward graph built before the clock starts: backward alone
  (c) forward    reweight_tensor, for scale: the pass (a) is the adjoint of, with the refresh's launches behind it
  (d) step       one unrolled IRLS step, forward + backward, through WeightedSolver.reweight_grad + solve_grad ...
  (d') step_torch  ... and the same with the weights restated in torch ((b)'s route) in front of solve_grad(wx=, wy=)
  (e) refresh    refresh_weights_tensor alone on ready planes: the redundant refresh solve_grad(wx=, wy=) makes after a
                 reweight_grad that has installed the same values
Before the timing the gradients of (a) are compared with those of (b) (max relative difference, reported).  There is no pass
threshold.  One JSON line per case, appended to --out.

Not measured here: EDGE coupling, the other penalties, the robust data term, one operator per channel, float32 views."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from coursecomputationalphotography_amd import tensor_ops
from reweight_bench import torch_weights

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, EPSILON, SCALE, CAP, TOL = 1e-2, 1e-2, 0.75, 8, 1e-6
PENALTY, COUPLING = "charbonnier", "pixel"
WANT = ("u", "gx", "gy", "base_wx", "base_wy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r41_reweight_adjoint_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reweight_adjoint_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        bwx, bwy = ((0.5 + 1.5 * torch.rand(H, W, generator=gen, dtype=torch.float64)).to(dev) for _ in range(2))
        gx, gy = (torch.randn(H, W, Cn, generator=gen, dtype=torch.float32).to(dev) for _ in range(2))
        u = (255.0 * torch.rand(H, W, Cn, generator=gen, dtype=torch.float64)).to(dev)
        Gwx, Gwy = (torch.randn(H, W, generator=gen, dtype=torch.float64).to(dev) for _ in range(2))
        G = torch.randn(H, W, Cn, generator=gen, dtype=torch.float64).to(dev)
        s = tensor_ops.WeightedSolver(H, W, Cn, dev, iterations=CAP, epsilon=0.0)
        s.set_operator(bwx, bwy, LAMBDA)
        s.set_stop(relative=TOL)
        g, lam = s.grid, s._operator[2]
        out = {n: torch.empty((H, W) if n.startswith("base") else (H, W, Cn), dtype=torch.float32 if n in ("gx", "gy") else torch.float64,
                              device=dev) for n in WANT}
        leaves = [t.clone().requires_grad_(True) for t in (u, gx, gy, bwx, bwy)]
        twx, twy = torch_weights(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], PENALTY, COUPLING, SCALE, EPSILON)
        ready = (twx.detach().clone(), twy.detach().clone())

        def leg_adjoint():
            g.reweight_adjoint_tensor(PENALTY, COUPLING, SCALE, EPSILON, u, gx=gx, gy=gy, base_wx=bwx, base_wy=bwy, grad_wx=Gwx, grad_wy=Gwy,
                                      want=WANT, out=out)

        def leg_autograd():
            return torch.autograd.grad((twx, twy), leaves, (Gwx, Gwy), retain_graph=True)

        def leg_forward():
            g.reweight_tensor(PENALTY, COUPLING, SCALE, EPSILON, u=u, gx=gx, gy=gy, base_wx=bwx, base_wy=bwy, lam=lam)

        def step(route):
            t = [v.clone().requires_grad_(True) for v in (u, gx, gy, bwx, bwy)]
            if route == "fused":
                wx, wy = s.reweight_grad(PENALTY, COUPLING, SCALE, EPSILON, t[0], gx=t[1], gy=t[2], base_wx=t[3], base_wy=t[4], data_weight=lam)
            else:
                wx, wy = torch_weights(t[0], t[1], t[2], t[3], t[4], PENALTY, COUPLING, SCALE, EPSILON)
            x, _ = s.solve_grad(t[1], t[2], u, x0=u, wx=wx, wy=wy)
            x.backward(G)
            return t

        def leg_refresh():
            g.refresh_weights_tensor(ready[0], ready[1], lam)

        # (a) against (b) before the clock: the same gradients up to the rounding of two operation orders
        leg_adjoint()
        ref = leg_autograd()
        torch.cuda.synchronize()
        differs = {n: float(((out[n].to(torch.float64) - r.to(torch.float64)).abs().max() / r.abs().max()).item()) for n, r in zip(WANT, ref)}
        del ref
        legs = {"adjoint": leg_adjoint, "autograd": leg_autograd, "forward": leg_forward, "step": lambda: step("fused"),
                "step_torch": lambda: step("torch"), "refresh": leg_refresh}

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
        row = {"case": name, "penalty": PENALTY, "coupling": COUPLING, "pcg_iterations_cap": CAP, "a_differs_from_b_relative": differs}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
            row[f"{k}_spread"] = max(v) / min(v)
        row["a_over_b"] = row["adjoint_ms_best"] / row["autograd_ms_best"]
        row["a_over_c"] = row["adjoint_ms_best"] / row["forward_ms_best"]
        row["d_over_d_torch"] = row["step_ms_best"] / row["step_torch_ms_best"]
        row["e_share_of_d"] = row["refresh_ms_best"] / row["step_ms_best"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        del twx, twy, leaves
        s.close()


if __name__ == "__main__":
    main()
