#!/usr/bin/env python3
"""Differentiating IRLS at its fixed point against unrolling it, on one MI355X: tools/reweight_bench.py's protocol -- a random
image in [0, 200], zero guidance, a shared f64 operator, charbonnier / pixel (TV), at 752x566x3 and 4096^2 x3; wall time
(time.perf_counter) of each leg ending with the stream idle, one untimed run of each, then --rounds alternations in which
every leg runs three times and its best counts.

The state: --outer steps of irls_solve's loop, the reweight from the result, then the backward's start (the adjoint
right-hand side and its solve) and --advance steps of the z iteration; b and x are saved there and put back, outside the
clock, before every timed leg of (1) and (2).

  (1) the step alone:   (a) fused         irls_adjoint_step_tensor with its report: two launches
                        (b) four_calls    the gradient pass into ready float64 planes, the reweight adjoint's g_u into a ready
                                          tensor, G + g_u and the two sums of squares in torch, adjoint_begin_tensor
  (2) a backward step:  (c) warm          (a) and the enqueue solve from the x the previous solve left
                        (d) cold          (b) -- which zeroes x -- and the same solve; the PCG iterations of both per channel
  (3) a whole backward: (e) implicit      irls_solve_implicit(backward_steps = outer).backward
                        (f) unrolled      irls_solve_grad(outer).backward
  (4) torch.cuda.max_memory_allocated over forward + backward of (e) and (f), beyond what was allocated before.
There is no pass threshold.  One JSON line per case, appended to --out.

Not measured here: EDGE coupling, the other penalties, the robust data term, one operator per channel, float32 views, an
image with structure (the step counts of a converged loop), backward_tolerance's read-backs."""
import argparse, gc, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from coursecomputationalphotography_amd import tensor_ops

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
STRENGTH, EPSILON, CAP, TOL = 4.0, 0.5, 30, 1e-6
PENALTY, COUPLING = "charbonnier", "pixel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--outer", type=int, default=8)
    ap.add_argument("--advance", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r42_fixed_point_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fixed_point_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, Cn = CASES[name]
        gen = torch.Generator(device="cpu").manual_seed(7)
        f = (200.0 * torch.rand(H, W, Cn, generator=gen, dtype=torch.float64)).to(dev)
        G = torch.randn(H, W, Cn, generator=gen, dtype=torch.float64).to(dev)
        s = tensor_ops.WeightedSolver(H, W, Cn, dev, iterations=CAP, epsilon=0.0)
        s.set_operator(None, None, 1.0)
        s.set_stop(relative=TOL)
        g, lam = s.grid, s._operator[2]
        u = f
        for k in range(a.outer):
            s.reweight(PENALTY, COUPLING, STRENGTH, EPSILON, u=f if k == 0 else None, data_weight=lam)
            u, _ = s.solve(None, None, f, x0=u)
        s.reweight(PENALTY, COUPLING, STRENGTH, EPSILON, u=u, data_weight=lam)
        report, solve_report = torch.zeros((Cn, 2), dtype=torch.float64, device=dev), torch.zeros((Cn, 8), dtype=torch.float64, device=dev)
        planes = {n: torch.empty((H, W), dtype=torch.float64, device=dev) for n in ("wx", "wy")}
        g_u = {"u": torch.empty((H, W, Cn), dtype=torch.float64, device=dev)}
        z, sums = torch.empty((H, W, Cn), dtype=torch.float64, device=dev), torch.zeros((Cn, 2), dtype=torch.float64, device=dev)

        def fused():
            g.irls_adjoint_step_tensor(PENALTY, COUPLING, STRENGTH, EPSILON, u, G, lam=lam, report=report)

        def four_calls():
            z_old = g.get_b_tensor(out=z)                    # (the norm of the change needs the old z: one more copy)
            g.weighted_adjoint_tensor(u, None, None, None, None, want=("wx", "wy"), out=planes)
            g.reweight_adjoint_tensor(PENALTY, COUPLING, STRENGTH, EPSILON, u, lam=lam, grad_wx=planes["wx"], grad_wy=planes["wy"],
                                      want=("u",), out=g_u)
            new = G + g_u["u"]
            sums[:, 0] = (new - z_old).pow(2).sum(dim=(0, 1))
            sums[:, 1] = new.pow(2).sum(dim=(0, 1))
            g.adjoint_begin_tensor(new)

        g.adjoint_begin_tensor(G)
        s._enqueue_pcg(None)
        for _ in range(a.advance):
            fused()
            s._enqueue_pcg(None)
        torch.cuda.synchronize()
        b0, x0 = g.get_b_tensor(), g.get_x_tensor()

        def restore():
            g.set_b_tensor(b0)
            g.set_x_tensor(x0)

        iterations = {}

        def with_solve(step, key):
            def leg():
                step()
                s._enqueue_pcg(solve_report)
            leg.after = lambda: iterations.__setitem__(key, [int(v) for v in solve_report[:, 0].tolist()])
            return leg

        def whole(fn, **kw):
            image = f.clone().requires_grad_(True)
            x = fn(None, None, image, a.outer, CAP, penalty=PENALTY, coupling=COUPLING, strength=STRENGTH, epsilon=EPSILON, tolerance=TOL,
                   strict=False, **kw)
            return lambda: x.backward(G, retain_graph=True)

        legs = {"fused": fused, "four_calls": four_calls, "warm": with_solve(fused, "warm"), "cold": with_solve(four_calls, "cold")}

        def timed(fn, prepare=None):
            if prepare:
                prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if hasattr(fn, "after"):
                fn.after()
            return ms

        for fn in legs.values():                             # one untimed run of every leg
            timed(fn, restore)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(min(timed(fn, restore) for _ in range(3)))
        # the two routes leave the same z (bit for bit) before their solves
        restore()
        fused()
        one = g.get_b_tensor()
        restore()
        four_calls()
        same_bits = bool(torch.equal(one, g.get_b_tensor()))
        s.close()
        del one, b0, x0, z, g_u, planes
        # (3) and (4): whole backwards, each on its own solver; the peak over forward + backward beyond the standing allocations
        row = {"case": name, "penalty": PENALTY, "coupling": COUPLING, "pcg_iterations_cap": CAP, "tolerance": TOL, "outer": a.outer,
               "advance": a.advance, "fused_equals_four_calls_bits": same_bits, "solve_iterations": iterations}
        routes = {"implicit": (tensor_ops.irls_solve_implicit, dict(backward_steps=a.outer)), "unrolled": (tensor_ops.irls_solve_grad, {})}
        whole_ms = {k: [] for k in routes}
        for k, (fn, kw) in routes.items():
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            back = whole(fn, **kw)
            timed(back)                                      # the untimed run, inside the peak
            row[f"{k}_peak_bytes"] = torch.cuda.max_memory_allocated(dev) - before
            for _ in range(a.rounds):
                whole_ms[k].append(min(timed(back) for _ in range(3)))
            del back
        for k, v in list(times.items()) + list(whole_ms.items()):
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
            row[f"{k}_spread"] = max(v) / min(v)
        row["a_over_b"] = row["fused_ms_best"] / row["four_calls_ms_best"]
        row["c_over_d"] = row["warm_ms_best"] / row["cold_ms_best"]
        row["a_share_of_c"] = row["fused_ms_best"] / row["warm_ms_best"]
        row["e_over_f"] = row["implicit_ms_best"] / row["unrolled_ms_best"]
        row["peak_e_over_f"] = row["implicit_peak_bytes"] / row["unrolled_peak_bytes"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
