#!/usr/bin/env python3
"""The host-free multigrid PCG (ccp_grid_mg_prepare + ccp_grid_mg_conjugate_gradient_enqueue) against the synchronous call
on one MI355X: a weighted handle with unit weights, lambda = 1e-2, the rescaled hierarchy, at 752x566x3 (the reference's own
image size: a solve there is launches, not bytes) and 4096^2 x3.  The system is manufactured (b = A x*, x* uniform [0, 255));
every timed solve starts from x = 0, and max_iteration is the count the synchronous call needs to 1e-10 |b| (the largest
reported `iterations` over the channels, plus the one update that passes epsilon), so the enqueue call queues no iteration
the synchronous call does not also run on some channel.

Three legs, each the wall time of one solve that ends in a stream synchronise (time.perf_counter around it):
  (a) sync     fill x = 0 + mg_conjugate_gradient (it waits for its own reports)
  (b) enqueue  fill x = 0 + mg_conjugate_gradient_enqueue + torch.cuda.synchronize
  (c) graph    one torch.cuda.graph replay of right-hand-side assembly + enqueue solve + read-out of x
               (tensor_ops.WeightedSolver.solve into static tensors) + torch.cuda.synchronize; for comparison
               (c_eager) is the same pipeline enqueued call by call.
One untimed run of every leg, then the legs alternated a, b, c, c_eager --rounds times in one process; per leg the best
and all the times are reported, and (a)'s own spread is the noise floor.  One JSON line per case, appended to --out."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from coursecomputationalphotography_amd import capi, tensor_ops

CASES = {"752x566x3": (752, 566, 3), "4096x4096x3": (4096, 4096, 3)}
LAMBDA, SWEEPS = 1e-2, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r29_enqueue_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("enqueue_bench: no GPU (this tool measures; it does not fall back)")
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
        _, bb = g.residual_norm2()
        eps = 1e-10 * float(max(bb)) ** 0.5
        g.fill_x(0.0)
        reps = g.mg_conjugate_gradient(eps, 200, SWEEPS)
        # `iterations` counts the completed iterations (the beta steps); the update whose residual passes epsilon is one
        # more, so the cap that still converges is the count + 1
        cap = max(r.iterations for r in reps) + 1
        g.fill_x(0.0)
        reps = g.mg_conjugate_gradient(eps, cap, SWEEPS)
        assert all(r.converged for r in reps), [r.iterations for r in reps]
        x_sync = g.get_x_tensor()
        g.mg_prepare(SWEEPS)
        report = torch.zeros((Cn, 6), dtype=torch.float64, device=dev)

        def leg_sync():
            g.fill_x(0.0)
            g.mg_conjugate_gradient(eps, cap, SWEEPS)

        def leg_enqueue():
            g.fill_x(0.0)
            g.mg_conjugate_gradient_enqueue(eps, cap, SWEEPS, report)

        # the pipeline of (c): the same operator on a persistent handle, f = the manufactured x*, zero guidance
        solver = tensor_ops.WeightedSolver(H, W, Cn, dev, iterations=cap, epsilon=eps)
        solver.set_operator(one, one, lam)
        g.randomize_x(1, 0.0, 255.0)
        f = g.get_x_tensor()
        out = torch.zeros(H, W, Cn, dtype=torch.float64, device=dev)
        preport = torch.zeros((Cn, 6), dtype=torch.float64, device=dev)

        def leg_eager():
            solver.solve(None, None, f, out=out, report=preport)

        leg_eager()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                leg_eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        legs = {"sync": leg_sync, "enqueue": leg_enqueue, "graph": graph.replay, "pipeline_eager": leg_eager}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for fn in legs.values():                             # one untimed run of every leg
            timed(fn)
        # the enqueue solve gave the synchronous solve's x (the last enqueue leg ran from x = 0 on the same b)
        leg_enqueue()
        torch.cuda.synchronize()
        same = bool(torch.equal(g.get_x_tensor().view(torch.int64), x_sync.view(torch.int64)))
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        row = {"case": name, "max_iteration": cap, "iterations": [r.iterations for r in reps], "epsilon": eps,
               "enqueue_x_equals_sync_bits": same, "pipeline_iterations": preport[:, 0].tolist(),
               "pipeline_converged": preport[:, 1].tolist()}
        for k, v in times.items():
            row[f"{k}_ms_best"] = min(v)
            row[f"{k}_ms_all"] = v
        row["enqueue_over_sync"] = row["enqueue_ms_best"] / row["sync_ms_best"]
        row["graph_over_pipeline_eager"] = row["graph_ms_best"] / row["pipeline_eager_ms_best"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        del graph
        solver.close()
        g.close()


if __name__ == "__main__":
    main()
