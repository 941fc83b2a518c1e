#!/usr/bin/env python3
"""The backward pass of a weighted solve on one MI355X (capi.Grid.adjoint_begin_tensor / weighted_adjoint_tensor): WLS
edge-preserving smoothing (tools/weighted_bench.py's image, lambda 1, alpha 1.2) at 752x566 x 3 and 4096^2 x 3, and the
screened constrained ellipse of tools/constrained_bench.py (lambda = 1e-2, wx = wy = 1, every pixel outside the central
ellipse fixed) at 4096^2 x 3, all on the rescaled hierarchy.

Per case one handle runs --rounds rounds (default 6: three, and a repeat of the three for the spread) of
    forward:  assemble b, x := f; MG-PCG to 1e-10 |b| or --max-iterations;  u := x
    adjoint:  adjoint_begin(G);   MG-PCG to the same epsilon and cap           (G: seeded uniform, scaled to |G| = |b| so that
              the one epsilon is the same relative tolerance for both solves)
    pass:     weighted_adjoint_tensor, --pass-repeats times between two events, the best taken (a short spin kernel in front
              keeps the device busy while the host enqueues, so the events enclose the pass and no idle time)
and prints one JSON line per round, then a summary: the best and the spread (max - min) of the forward ms, the adjoint ms
and the pass ms over the rounds, the adjoint / forward ratio of the bests, and the pass's byte model.  Solve times are the
device times of the reports (HIP events around the PCG loops), summed over the channels.

Byte model of the pass, per pixel: the element bytes of every view passed whose strides are not all zero (a broadcast
scalar is one element, read from the cache) times its channel count, inputs and outputs, plus 8 C for x.  Neighbour
re-reads are expected to hit the cache and are not counted.  bytes_per_s = model * pixels / best pass time; the pool's
measured streaming ceiling is 5.3-5.5 TB/s (profiles/r03_hbm_calib.txt)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
from coursecomputationalphotography_amd import capi, tensor_ops

CASES = {"wls_752x566_x3": (752, 566, 3, "wls"), "wls_4096sq_x3": (4096, 4096, 3, "wls"), "ellipse_4096sq_x3": (4096, 4096, 3, "ellipse")}


def image(W, H, C, dev):
    """tools/weighted_bench.py's image: flat patches of 16 px with hard edges plus a little noise, u8."""
    g = torch.Generator(device=dev).manual_seed(7)
    patches = torch.rand((H // 16 + 1, W // 16 + 1, C), generator=g, device=dev)
    img = patches.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W] * 230.0
    img = img + 25.0 * torch.rand((H, W, C), generator=g, device=dev)
    return img.clamp(0, 255).to(torch.uint8)


def ellipse_outside(W, H, dev):
    """u8 H x W, 1 outside the central ellipse with half-axes 0.4 W and 0.4 H (tools/constrained_bench.py)."""
    y = (torch.arange(H, device=dev, dtype=torch.float32) - (H - 1) / 2) / (0.4 * H)
    x = (torch.arange(W, device=dev, dtype=torch.float32) - (W - 1) / 2) / (0.4 * W)
    return ((y * y)[:, None] + (x * x)[None, :] >= 1.0).to(torch.uint8)


def view_bytes(t, C):
    """Bytes per pixel a view contributes to the model: 0 for None and for a broadcast scalar."""
    if t is None or all(s == 0 for s in t.stride()):
        return 0
    return t.element_size() * (C if t.dim() == 3 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pass-repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        W, H, C, kind = CASES[name]
        gen = torch.Generator(device=dev).manual_seed(11)
        one = lambda v: torch.tensor(v, dtype=torch.float64, device=dev).expand(H, W)
        gx = gy = values = mask = None
        if kind == "wls":
            f = image(W, H, C, dev).to(torch.float64)
            wx, wy = tensor_ops.wls_weights(f / 255.0, lam=1.0, alpha=1.2, eps=1e-4)
            lam = one(1.0)
            want = ("wx", "wy", "lam", "f")                  # what a learner of edge weights and lambda asks for
        else:
            gx = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
            gy = (torch.rand((H, W, C), generator=gen, device=dev) - 0.5) * 16.0
            f = torch.rand((H, W, C), generator=gen, device=dev, dtype=torch.float64) * 255.0
            values = torch.rand((H, W, C), generator=gen, device=dev, dtype=torch.float64) * 255.0
            mask = ellipse_outside(W, H, dev)
            wx, wy, lam = None, None, one(1e-2)
            want = ("wx", "wy", "lam", "gx", "gy", "f", "values")
        G = torch.rand((H, W, C), generator=gen, device=dev, dtype=torch.float64) - 0.5
        g = capi.Grid(W, H, C, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights_tensor(wx, wy, lam, fixed=mask)
        g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=True)
        _, bb = g.residual_norm2()
        b_norm = float(np.sqrt(bb.sum()))
        eps = 1e-10 * b_norm
        G = G * (b_norm / float(G.norm()))
        outs = {n: torch.empty((H, W) if n in ("wx", "wy", "lam") else (H, W, C), dtype=torch.float64, device=dev) for n in want}
        need_grad = G if "values" in want else None
        model = 8 * C + sum(view_bytes(t, C) for t in (f, gx, gy, wx, wy, lam, mask, need_grad)) + 8 * C  # x, the inputs, u
        model += sum(view_bytes(t, C) for t in outs.values())
        rounds = []
        for r in range(a.rounds):
            g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=True)
            fwd = g.mg_conjugate_gradient(eps, a.max_iterations, 2)
            u = g.get_x_tensor()
            g.adjoint_begin_tensor(G)
            adj = g.mg_conjugate_gradient(eps, a.max_iterations, 2)
            best = None
            for _ in range(a.pass_repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(5_000_000)                 # keeps the device busy while the host enqueues: no idle time between the events
                e0.record()
                g.weighted_adjoint_tensor(u, need_grad, gx, gy, f, wx, wy, lam, mask, want=want, out=outs)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                best = ms if best is None else min(best, ms)
            rec = {"case": name, "round": r, "width": W, "height": H, "channels": C, "max_iterations": a.max_iterations, "epsilon": eps,
                   "forward_iterations": [x.iterations for x in fwd], "forward_converged": [bool(x.converged) for x in fwd],
                   "forward_ms": 1e3 * sum(x.seconds for x in fwd),
                   "adjoint_iterations": [x.iterations for x in adj], "adjoint_converged": [bool(x.converged) for x in adj],
                   "adjoint_ms": 1e3 * sum(x.seconds for x in adj), "pass_ms": best}
            rounds.append(rec)
            print(json.dumps(rec), flush=True)
        col = lambda k: [r[k] for r in rounds]
        best_pass = min(col("pass_ms"))
        summary = {"case": name, "summary": True, "rounds": len(rounds), "gradients": list(want),
                   "forward_iterations": rounds[0]["forward_iterations"], "adjoint_iterations": rounds[0]["adjoint_iterations"]}
        for k in ("forward_ms", "adjoint_ms", "pass_ms"):
            summary["best_" + k] = min(col(k))
            summary["spread_" + k] = max(col(k)) - min(col(k))
        summary["adjoint_over_forward"] = summary["best_adjoint_ms"] / summary["best_forward_ms"]
        fi, ai = sum(i + 1 for i in rounds[0]["forward_iterations"]), sum(i + 1 for i in rounds[0]["adjoint_iterations"])
        summary["adjoint_over_forward_per_iteration"] = (summary["best_adjoint_ms"] / ai) / (summary["best_forward_ms"] / fi)
        summary["pass_bytes_per_pixel"] = model
        summary["pass_bytes_per_s"] = model * W * H / (best_pass * 1e-3)
        print(json.dumps(summary), flush=True)
        g.close()
        del f, G, outs, u
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
