"""GPU: a whole robust IRLS loop in one graph.  On 70 x 40 x 3, torch.cuda.graph records 3 x (WeightedSolver.reweight with a
robust data term, the assembly, the enqueue solve) and the read-outs, all from static tensors, and the graph is replayed on
two different images.  Each replay equals, bit for bit, the eager loop on a fresh WeightedSolver: x and the report of every
step and the final wx, wy and lambda.  f64, f32 and a per-channel batched operator.

As tests/test_gpu_reweight_graph.py, whose inputs this file uses: the capture runs in the default error mode, so it is also
the proof that the call neither synchronises nor allocates; the graph is one linear chain on the capturing side stream; no
queue or graph environment variable is set."""
import pytest
import torch

import test_gpu_reweight_graph as rg
from coursecomputationalphotography_amd import tensor_ops

pytestmark = pytest.mark.gpu

DEV, W, H, Cn, CAP, OUTER, MODES = rg.DEV, rg.W, rg.H, rg.Cn, rg.CAP, rg.OUTER, rg.MODES
DATA_SCALE, DATA_EPSILON = 0.5, 4.0                            # the images are in [0, 255] with noise of 8
bits = rg.bits


def loop(solver, b, gx, gy, f, outs, reports, wout):
    """OUTER x (reweight, assemble + enqueue solve + read-out); the first step reweights from f with the quadratic data
    term, the later ones from x with the Charbonnier one: irls_solve's steps"""
    x = f
    for k in range(OUTER):
        solver.reweight("charbonnier", "pixel", rg.STRENGTH, rg.EPSILON, u=f if k == 0 else None, gx=gx, gy=gy, base_wx=b[0], base_wy=b[1],
                        data_weight=b[2], out=wout, data_penalty="quadratic" if k == 0 else "charbonnier", data_scale=DATA_SCALE,
                        data_epsilon=DATA_EPSILON, f=f)
        x, _ = solver.solve(gx, gy, f, x0=x, out=outs[k], report=reports[k])


def buffers(mode):
    outs, reports, wout = rg.buffers(mode)
    return outs, reports, wout + (torch.full_like(wout[0], -1.0),)


@pytest.mark.parametrize("mode", list(MODES))
def test_captured_robust_loop_replays_the_eager_loop(mode):
    b = rg.base(mode, 41)
    imgs = [rg.image(51), rg.image(52)]
    eager = []
    for gx, gy, f in imgs:                                     # the reference: a fresh solver, the loop issued eagerly
        with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=CAP, epsilon=0.0, **MODES[mode]) as fresh:
            fresh.set_operator(*b)
            fresh.set_stop(relative=rg.TOL)
            outs, reports, wout = buffers(mode)
            loop(fresh, b, gx, gy, f, outs, reports, wout)
            torch.cuda.synchronize()
            eager.append((outs, reports, wout))
    assert not torch.equal(eager[0][0][-1], eager[1][0][-1])
    assert not torch.equal(eager[0][0][0], eager[0][0][-1])     # the outer steps move the solution
    with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=CAP, epsilon=0.0, **MODES[mode]) as solver:
        solver.set_operator(*rg.base(mode, 40))                # prepared, on other weights
        solver.set_stop(relative=rg.TOL)
        sgx, sgy, sf = (torch.zeros_like(t) for t in imgs[0])  # static: the graph reads the image from them
        outs, reports, wout = buffers(mode)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):         # the default capture error mode
                loop(solver, b, sgx, sgy, sf, outs, reports, wout)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        for (gx, gy, f), (eouts, ereports, ewout) in zip(imgs, eager):
            sgx.copy_(gx), sgy.copy_(gy), sf.copy_(f)
            for t in outs:
                t.zero_()
            for t in reports + list(wout):
                t.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            print("replay: iterations", [r[:, 0].tolist() for r in reports], "converged", [r[:, 1].tolist() for r in reports])
            for k in range(OUTER):
                assert torch.equal(bits(outs[k]), bits(eouts[k])), (mode, "x of step", k)
                assert torch.equal(bits(reports[k]), bits(ereports[k])), (mode, "report of step", k)
                assert bool((reports[k][:, 5] == 0.0).all()) and bool((reports[k][:, 0] > 0).all())
            for name, got, want in zip(("wx", "wy", "lambda"), wout, ewout):
                assert torch.equal(bits(got), bits(want)), (mode, "the final", name)
            assert bool((wout[0][:, :-1] > 0).all()) and not bool(wout[0][:, -1].any())
            # the lambda of the last step is a robust one: below the base where the iterate left the data, never above phi_d(0)
            assert bool((wout[2] > 0).all()) and bool((wout[2] <= b[2].to(torch.float64) * (DATA_SCALE / DATA_EPSILON)).all())
            assert not torch.equal(wout[2], (b[2].to(torch.float64) * DATA_SCALE).expand_as(wout[2]))
        del graph
