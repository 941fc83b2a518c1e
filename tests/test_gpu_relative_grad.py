"""GPU: tensor_ops.WeightedSolver.set_stop -- the relative stop test (capi.Grid.mg_conjugate_gradient_enqueue_relative) in
solve_grad's forward and backward.

The system is the constrained 64x48x2 one of tests/test_gpu_mg_enqueue.py's solve_grad test.  The loss is
L = s sum(u q) with a fixed random q, at s = 1 and s = 2^-30: the adjoint right-hand side dL/du = s q scales exactly, and
with a threshold relative to |dL/du| the adjoint solve makes the same iterations on exactly scaled numbers, so every
gradient at s = 2^-30 is 2^-30 times the gradient at s = 1, bit for bit (a power of two commutes with every operation
of the solve and of the gradient pass, and with the rounding to a float32 gradient).  With the absolute epsilon the
backward solve at s = 2^-30 would start below its threshold and return after 0 iterations."""
import pytest
import torch

import mixed_helpers as mh
from coursecomputationalphotography_amd import tensor_ops
from replay_helpers import SENTINEL, screened

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
W, H, Cn, CAP = 64, 48, 2, 60
NAMES = ("gx", "gy", "f", "values", "wx", "wy", "data_weight")


def images(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    gx, gy = (torch.randn(H, W, Cn, generator=g, dtype=torch.float32).to(DEV) for _ in range(2))
    f = (255.0 * torch.rand(H, W, Cn, generator=g, dtype=torch.float64)).to(DEV)
    return gx, gy, f


@pytest.fixture(scope="module")
def system():
    wx, wy, lam = (torch.from_numpy(a).to(torch.float64).to(DEV) for a in screened(W, H, 78))
    fixed = torch.from_numpy(mh.ellipse_fixed(W, H)).to(DEV)
    gx, gy, f = images(2)
    values = images(3)[2]
    q = images(4)[2] / 255.0
    return dict(gx=gx, gy=gy, f=f, values=values, wx=wx, wy=wy, data_weight=lam, fixed=fixed, q=q)


def raw(t):
    return t.detach().contiguous().view(torch.uint8)


def run(solver, sys, s, fields, weights):
    """One forward and backward of L = s sum(u q): ({name: gradient}, report, adjoint report).  weights: the keyword form,
    which also differentiates with respect to wx, wy and data_weight."""
    names = NAMES if weights else NAMES[:4]
    a = {n: sys[n].clone().requires_grad_(True) for n in names}
    rep, arep = (torch.full((Cn, fields), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2))
    kw = {n: a[n] for n in names[4:]}
    u, _ = solver.solve_grad(a["gx"], a["gy"], a["f"], a["values"], x0=sys["f"], report=rep, adjoint_report=arep, **kw)
    (s * (u * sys["q"]).sum()).backward()
    torch.cuda.synchronize()
    return {n: a[n].grad for n in names}, rep, arep


@pytest.mark.parametrize("weights", [False, True], ids=["inputs", "weights"])
def test_gradients_scale_exactly_with_the_loss(system, weights):
    s = 2.0 ** -30
    with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=CAP, epsilon=1e-8) as solver:
        solver.set_operator(system["wx"], system["wy"], system["data_weight"], system["fixed"])
        solver.set_stop(0.0, 1e-10)
        g1, rep1, arep1 = run(solver, system, 1.0, 8, weights)
        gs, reps, areps = run(solver, system, s, 8, weights)
        print("forward iterations", rep1[:, 0].tolist(), "adjoint iterations", arep1[:, 0].tolist(), areps[:, 0].tolist(),
              "adjoint |b|", arep1[:, 6].tolist(), areps[:, 6].tolist())
        assert torch.equal(raw(reps), raw(rep1))                 # the forward solve does not see the loss
        assert torch.equal(areps[:, 0], arep1[:, 0])
        for arep in (arep1, areps):
            assert bool((arep[:, 1] == 1.0).all()) and bool((arep[:, 0] >= 1).all()) and bool((arep[:, 0] < CAP).all()), arep
        assert torch.equal(raw(areps[:, 6]), raw(arep1[:, 6] * s)) and torch.equal(raw(areps[:, 7]), raw(arep1[:, 7] * s))
        for n, g in g1.items():
            assert g is not None and gs[n] is not None and gs[n].dtype == g.dtype, n
            assert bool(g.abs().max() > 0), n
            assert torch.equal(raw(gs[n]), raw(g * s)), n


def test_relative_none_is_the_solver_as_it_was(system):
    with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=CAP, epsilon=1e-8) as solver:
        solver.set_operator(system["wx"], system["wy"], system["data_weight"], system["fixed"])
        g0, rep0, arep0 = run(solver, system, 1.0, 6, True)      # before set_stop was ever called
        solver.set_stop(0.0, 1e-10)
        run(solver, system, 1.0, 8, True)
        solver.set_stop(1e-8, None)
        g1, rep1, arep1 = run(solver, system, 1.0, 6, True)
        assert torch.equal(raw(rep1), raw(rep0)) and torch.equal(raw(arep1), raw(arep0))
        assert bool((arep0[:, 1] == 1.0).all())
        for n, g in g0.items():
            assert torch.equal(raw(g1[n]), raw(g)), n
        with pytest.raises(ValueError):                          # the report's width follows the stop test
            solver.solve(system["gx"], system["gy"], system["f"], system["values"],
                         report=torch.zeros(Cn, 8, dtype=torch.float64, device=DEV))
