"""GPU: tensor_ops.irls_solve_implicit (irls_solve's loop under no_grad, then WeightedSolver.fixed_point_grad) on 16 x 12 x 2.

Against the dense model.  TV (Charbonnier / pixel), Huber / edge and TV-L1, each with base weights, a data_weight plane and
three fixed pixels; `outer` and `backward_steps` are the step counts tests/test_fixed_point_helpers.py asserts of the dense
loops (fixed_point_helpers.STEPS) plus a margin of 5.  The value has irls_solve's bits, and every gradient -- f, gx, gy,
values, the base wx / wy, the data_weight plane, a 0-dim strength -- is compared with
fixed_point_helpers.dense_fixed_point_gradients.

Tolerance, measured on the CPU and not against the code under test: the gap, max |a - b| / max |b| per gradient, between
the dense loop b and the same loop a with every solve, forward and adjoint, done by the numpy model of the device's
multigrid PCG (fixed_point_helpers.pcg_hooks) at this test's relative tolerance 1e-10.  Measured worst over the three cases
and the strength: 1.44e-8 (TV-L1, d/ddata_weight; TV 7.6e-9, Huber 4.1e-9, d/dstrength 1.4e-9); allowed: 10 x that, 1.44e-7.
A float32 gradient (gx, gy) is the sum of two terms -- the gradient pass's and the reweight adjoint's, taken once -- so the
format's (4 steps - 1) 2^-24 of tests/test_gpu_irls_grad.py is 3 x 2^-24 here (steps = 1).  NOTES R42.1 has the figures.

Against the unrolled gradient.  With outer = 40 (TV: 35 steps reach an update of 1e-12; TV-L1: 19) the implicit gradient
agrees with irls_solve_grad's to the same tolerance: two routes to one quantity.  (irls_solve_grad's own float32 gradients are
float32 sums of 2 x 40 terms: they bring their (4 x 40 - 1) 2^-24 along, as tests/test_gpu_irls_grad.py works out.)

backward_tolerance ends the loop early, and with strict and a cap of 2 raises.  After the forward, torch's allocated memory
does not grow with `outer` beyond one canvas-sized tensor, while irls_solve_grad's does.  A forward, a second forward with
other weights on the same solver, then the first's backward gives the first's gradients bit for bit."""
import gc

import numpy as np
import pytest
import torch

import fixed_point_helpers as fp
from coursecomputationalphotography_amd import tensor_ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
W, H, ITER, TOL = 16, 12, 80, 1e-10
PCG_GAP = 1.44e-8                                              # measured on the CPU (the docstring)
ALLOWED = 10.0 * PCG_GAP
F32 = 3 * 2.0 ** -24                                           # one float32 sum of two float32-sized terms (the docstring)
WRT = {"f": "f", "gx": "gx", "gy": "gy", "values": "values", "wx": "base_wx", "wy": "base_wy", "lam": "data_weight"}


def dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


_REFERENCE = {}


def reference(name, strength_in_base=False):
    """(inputs, (u, gradients, info)) of the dense model, computed once per case and shared; never modified"""
    key = (name, strength_in_base)
    if key not in _REFERENCE:
        penalty, coupling = fp.CASES[name][:2]
        a = fp.case_inputs(name, W, H)
        kw = fp.case_kw(name, a)
        scale = fp.STRENGTH
        if strength_in_base:                                     # a 0-dim tensor strength: folded into both bases, scale 1
            kw.update(base_wx=fp.STRENGTH * a["wx"], base_wy=fp.STRENGTH * a["wy"])
            scale = 1.0
        forward, backward = fp.STEPS[name]
        _REFERENCE[key] = (a, fp.dense_fixed_point_gradients(a["G"], a["f"], a["gx"].astype(np.float64), a["gy"].astype(np.float64), penalty,
                                                             coupling, scale, fp.EPS, forward + fp.MARGIN, backward + fp.MARGIN, **kw))
    return _REFERENCE[key]


def device_run(name, a, outer, requires=(), strength=fp.STRENGTH, fn=None, **kw):
    penalty, coupling, robust = fp.CASES[name][:3]
    t = {n: dev(a[n]) for n in ("f", "gx", "gy", "lam", "wx", "wy", "values", "fixed")}
    for n in requires:
        t[n].requires_grad_(True)
    kw = dict(dict(penalty=penalty, coupling=coupling, strength=strength, epsilon=fp.EPS, data_weight=t["lam"], wx=t["wx"], wy=t["wy"],
                   fixed=t["fixed"], values=t["values"], tolerance=TOL), **kw)
    if robust:
        kw.update(data_penalty="charbonnier", data_epsilon=fp.DEPS)
    return (fn or tensor_ops.irls_solve_implicit)(t["gx"], t["gy"], t["f"], outer, ITER, **kw), t


@pytest.mark.parametrize("name", list(fp.CASES))
def test_value_and_gradients_match_the_dense_model(name):
    a, (u_ref, ref, _) = reference(name)
    forward, backward = fp.STEPS[name]
    history = []
    x, t = device_run(name, a, forward + fp.MARGIN, requires=tuple(WRT), backward_steps=backward + fp.MARGIN, backward_history=history)
    plain, _ = device_run(name, a, forward + fp.MARGIN, fn=tensor_ops.irls_solve)
    assert x.grad_fn is not None and x.dtype == torch.float64 and torch.equal(x.detach(), plain)
    assert fp.relative_gap(x.detach().cpu().numpy(), u_ref) <= ALLOWED
    x.backward(dev(a["G"]))
    assert len(history) == backward + fp.MARGIN and all(tuple(r.shape) == (2, 2) for r in history)
    assert float(history[-1][:, 0].sum()) < float(history[0][:, 0].sum()) * 1e-12
    for n, m in WRT.items():
        g = t[n].grad
        assert g is not None and g.dtype == t[n].dtype and g.shape == t[n].shape, (name, n)
        gap = fp.relative_gap(g.cpu().numpy(), ref[m])
        print(f"{name}: d/d{n} differs from the dense model by {gap:.3g}")
        assert gap <= ALLOWED + (F32 if g.dtype == torch.float32 else 0.0), (name, n, gap)


def test_a_zero_dim_strength_gets_its_gradient():
    a, (_, ref, _) = reference("tv", strength_in_base=True)
    # base_wx = strength * wx and base_wy = strength * wy: d/dstrength = sum(g_base_wx * wx) + sum(g_base_wy * wy)
    expect = float((ref["base_wx"] * a["wx"]).sum() + (ref["base_wy"] * a["wy"]).sum())
    strength = torch.tensor(fp.STRENGTH, dtype=torch.float64, device=DEV, requires_grad=True)
    forward, backward = fp.STEPS["tv"]
    x, _ = device_run("tv", a, forward + fp.MARGIN, strength=strength, backward_steps=backward + fp.MARGIN)
    x.backward(dev(a["G"]))
    assert strength.grad is not None and strength.grad.dim() == 0
    gap = abs(float(strength.grad) - expect) / abs(expect)
    print(f"tv: d/dstrength differs from the dense model by {gap:.3g}")
    assert gap <= ALLOWED


@pytest.mark.parametrize("name", ["tv", "tv_l1"])
def test_the_implicit_gradient_is_the_unrolled_one_at_40_steps(name):
    a = fp.case_inputs(name, W, H)
    G = dev(a["G"])
    x, t = device_run(name, a, 40, requires=tuple(WRT))
    y, s = device_run(name, a, 40, requires=tuple(WRT), fn=tensor_ops.irls_solve_grad)
    assert torch.equal(x.detach(), y.detach())
    x.backward(G)
    y.backward(G)
    for n in WRT:
        gap = fp.relative_gap(t[n].grad.cpu().numpy(), s[n].grad.to(torch.float64).cpu().numpy())
        print(f"{name}: d/d{n} differs from irls_solve_grad's by {gap:.3g}")
        assert gap <= ALLOWED + (F32 + (4 * 40 - 1) * 2.0 ** -24 if t[n].grad.dtype == torch.float32 else 0.0), (name, n, gap)


def test_backward_tolerance_ends_the_loop_and_strict_raises_at_the_cap():
    a = fp.case_inputs("tv", W, H)
    G = dev(a["G"])
    history = []
    x, t = device_run("tv", a, 40, requires=("f",), backward_steps=200, backward_tolerance=1e-8, check_every=4, backward_history=history)
    x.backward(G)
    assert 0 < len(history) < 200 and len(history) % 4 == 0
    bound = (1e-8 * float(G.norm())) ** 2                        # (the loop forms it by another sum: a rounding of slack)
    assert float(history[-1][:, 0].sum()) <= bound * (1 + 1e-12) and float(history[len(history) - 5][:, 0].sum()) > bound * (1 - 1e-12)
    full, s = device_run("tv", a, 40, requires=("f",), backward_steps=60)
    full.backward(G)
    # z is then within rho / (1 - rho) 1e-8 |G| of its limit (rho about 0.45), v = A^-1 z with |A^-1| <= 1 / min lambda = 1.33, and
    # |G|_2 = 20 against a largest gradient entry of order 1: 1e-6 bounds the max-norm gap with a margin of 2 to 3
    assert fp.relative_gap(t["f"].grad.cpu().numpy(), s["f"].grad.cpu().numpy()) <= 1e-6
    x, _ = device_run("tv", a, 40, requires=("f",), backward_steps=2, backward_tolerance=1e-8)
    with pytest.raises(RuntimeError, match="did not reach backward_tolerance"):
        x.backward(G)
    x, t = device_run("tv", a, 40, requires=("f",), backward_steps=2, backward_tolerance=1e-8, strict=False)
    x.backward(G)                                                # ... and only then
    assert t["f"].grad is not None
    with pytest.raises(RuntimeError, match="still moves"):       # the forward's own check: 3 steps are not a fixed point
        device_run("tv", a, 3, requires=("f",))


def test_memory_after_forward_does_not_grow_with_outer():
    Wm, Hm = 64, 48
    a = fp.case_inputs("tv", Wm, Hm)
    canvas = Hm * Wm * 2 * 8

    def after_forward(fn, outer, **kw):
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        x, t = device_run("tv", a, outer, requires=("f", "wx"), fn=fn, strict=False, **kw)
        torch.cuda.synchronize()
        inputs = sum(v.numel() * v.element_size() for v in t.values() if v is not None)
        used = torch.cuda.memory_allocated(DEV) - base - inputs
        del x, t
        return used

    implicit = [after_forward(tensor_ops.irls_solve_implicit, k) for k in (4, 12)]
    unrolled = [after_forward(tensor_ops.irls_solve_grad, k) for k in (4, 12)]
    print(f"after forward, beyond the inputs: implicit {implicit} bytes, unrolled {unrolled} bytes at outer = 4, 12; a canvas is {canvas}")
    assert implicit[1] - implicit[0] <= canvas
    assert unrolled[1] - unrolled[0] >= 8 * canvas               # u per step alone; wx and wy come on top


def test_a_moved_operator_is_reinstalled():
    """a forward, a second forward with other weights on the same solver, then the first's backward: the first's bits"""
    cases = []
    for name, flip in (("tv", False), ("tv", True)):
        a = fp.case_inputs(name, W, H)
        if flip:
            a.update(f=a["f"][::-1].copy(), wx=a["wx"][:, ::-1].copy())
        u, _ = device_run(name, a, 40, fn=tensor_ops.irls_solve)
        cases.append((a, u))
    G = dev(cases[0][0]["G"])
    s = tensor_ops.WeightedSolver(H, W, 2, DEV, iterations=ITER, epsilon=0.0)
    first = cases[0][0]
    s.set_operator(dev(first["wx"]), dev(first["wy"]), dev(first["lam"]), dev(first["fixed"]))
    s.set_stop(relative=TOL)

    def attach(a, u):
        t = {n: dev(a[n]) for n in ("f", "gx", "gy", "lam", "wx", "wy", "values")}
        for n in ("f", "wx", "lam", "values"):
            t[n].requires_grad_(True)
        x = s.fixed_point_grad(u, "charbonnier", "pixel", fp.STRENGTH, fp.EPS, t["gx"], t["gy"], t["f"], t["values"], t["wx"], t["wy"], t["lam"],
                               backward_steps=12)
        return x, t

    x, t = attach(*cases[0])
    x.backward(G)
    alone = {n: t[n].grad.clone() for n in ("f", "wx", "lam", "values")}
    x, t = attach(*cases[0])
    y, _ = attach(*cases[1])                                     # moves the handle's operator
    x.backward(G)
    for n, g in alone.items():
        assert bool(g.any()) and torch.equal(t[n].grad, g), n
    s.close()
