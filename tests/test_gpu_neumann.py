"""GPU: CCP_MG_NULLSPACE_CONSTANT on weighted grid handles (include/ccp_gs.h, ccp_grid_mg_set_nullspace): the multigrid
PCG of a floating operator (lambda = 0, no fixed pixel, every in-canvas weight > 0) on the mean-free vectors.

Against tests/neumann_helpers.py: a consistent b converges in the model's iterations to the model's x (1e-6 max |x|, the
tolerance tests/test_gpu_weighted.py holds its MG-PCG to) and keeps the mean of the start vector to the rounding of one
n-term sum; b + 1e-3, on which the loop without the mode diverges (tests/test_neumann_helpers.py), converges in the same
iterations to the same x and reports mean(b); one V-cycle keeps the bits of the mode's existing V-cycle up to the mean
subtraction; what the mode does not serve is refused with x and b untouched and solves once repaired; a handle that went
through the mode and back gives the default's bits; per-channel operators equal one-channel handles bit for bit;
tensor_ops.integrate_gradients returns the image its exact differences came from."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import line_helpers as lh
import neumann_helpers as nh
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
SHAPES = [(64, 48), (257, 131), (3, 2), (33, 1)]
# (hierarchy, precision, smoother, smoothing sweeps)
MODES = {"galerkin": ("galerkin", "f64", "point", 2), "rescaled": ("rescaled", "f64", "point", 2),
         "f32": ("rescaled", "f32", "point", 2), "line": ("rescaled", "f64", "line", 1)}
CASES = [(W, H, weighted, mode) for W, H in SHAPES for weighted in (False, True) for mode in ("galerkin", "rescaled")]
# (the line smoother where a line-smoothed level has one row or column is refused, nh.line_served:
# test_line_smoother_with_a_one_row_level_is_refused)
CASES += [(W, H, True, mode) for W, H in SHAPES for mode in ("f32", "line") if mode != "line" or nh.line_served(W, H)]
CASES += [(64, 2, True, "line")]                                  # elongated, but its level 1 (32x1) is in the tail: served
CASES3 = [(257, 131, "galerkin"), (64, 48, "rescaled"), (33, 1, "rescaled")]   # three channels, random weights
# of b per channel, under one epsilon (1e-10 |b| of channel 0): x0 in [0, 255) gives |A x0| ~ 4 |b|, so only a larger b moves
# the first residual, and with it the stopping point (the model: 13, 15, 17 iterations at 257x131)
SCALES = (1.0, 30.0, 1000.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def exact_mean(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel()) / a.size


def mean_bound(x):
    """The rounding bound of one n-term sum: 2 n 2^-53 max |x|."""
    return 2 * x.size * 2.0 ** -53 * float(np.abs(x).max())


def close_to_model(x, want):
    """tests/test_gpu_weighted.py's comparison of an MG-PCG solution."""
    err = float(np.abs(x - want).max())
    return err, err <= 1e-6 * max(1.0, float(np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def model(W, H, weighted, mode, Cn):
    """(levels, wx, wy, [b per channel], [x0 per channel], epsilon, M, [the model's solve of b], [of b + 1e-3])"""
    kind, precision, smoother, nu = MODES[mode]
    levels, b, wx, wy, _, _ = nh.system(kind, W, H, weighted, seed=W + 3 * H)
    bs = [SCALES[c] * b for c in range(Cn)]
    x0 = [nh.rng(40 + c).uniform(0.0, 255.0, (H, W)) for c in range(Cn)]
    eps = 1e-10 * float(np.linalg.norm(b))
    M = nh.preconditioner(levels, kind, nu, precision, smoother)
    good = [nh.pcg(levels[0], M, bs[c], eps, 100, x0[c]) for c in range(Cn)]
    off = [nh.pcg(levels[0], M, bs[c] + 1e-3, eps, 100, x0[c]) for c in range(Cn)]
    return levels, wx, wy, bs, x0, eps, M, good, off


def handle(W, H, Cn, mode, wx=None, wy=None, lam=None, fixed=None):
    kind, precision, smoother, _ = MODES[mode]
    g = capi.Grid(W, H, Cn, weighted=True)
    g.mg_set_hierarchy(kind)
    g.mg_set_precision(precision)
    g.mg_set_smoother(smoother)
    g.mg_set_nullspace("constant")
    g.set_weights(wx, wy, lam, fixed=fixed)
    return g


def load(g, bs, xs):
    for c, (b, x) in enumerate(zip(bs, xs)):
        g.set_b(b, c)
        g.set_x(x, c)


def check_consistent(g, W, H, weighted, mode, Cn, what=""):
    """Test 1 on a handle that holds the case's operator: returns x per channel."""
    _, _, _, bs, x0, eps, _, good, _ = model(W, H, weighted, mode, Cn)
    load(g, bs, x0)
    reps = g.mg_conjugate_gradient(eps, 100, MODES[mode][3])
    out = []
    for c in range(Cn):
        want, n, conv, _, _ = good[c]
        x = g.get_x(c)
        err, ok = close_to_model(x, want)
        drift = abs(exact_mean(x) - exact_mean(x0[c]))
        print(f"{what}{W}x{H} {mode}{' weighted' if weighted else ''} channel {c}: {reps[c].iterations} iterations (model {n}), "
              f"|x - model| {err:.3e}, |mean(x) - mean(x0)| {drift:.3e} (bound {mean_bound(x):.3e})")
        assert conv and reps[c].converged, (c, reps[c].iterations)
        assert reps[c].iterations == n, (c, reps[c].iterations, n)
        assert ok, (c, err)
        assert drift <= mean_bound(x), (c, drift, mean_bound(x))
        assert np.array_equal(bits(g.get_b(c)), bits(bs[c]))         # b itself is not modified
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def device_solves(W, H, weighted, mode, Cn):
    """Both solves of a case on one handle: (x per channel of the consistent b, then reports, x and info of b + 1e-3)."""
    _, wx, wy, bs, x0, eps, _, _, _ = model(W, H, weighted, mode, Cn)
    g = handle(W, H, Cn, mode, wx, wy)
    with pytest.raises(capi.CcpError) as e:                          # no solve in the mode yet
        g.mg_nullspace_info(0)
    assert e.value.status == STATE
    good = check_consistent(g, W, H, weighted, mode, Cn)
    load(g, [b + 1e-3 for b in bs], x0)
    reps = g.mg_conjugate_gradient(eps, 100, MODES[mode][3])
    off = [g.get_x(c) for c in range(Cn)]
    info = [g.mg_nullspace_info(c) for c in range(Cn)]
    g.close()
    return good, [(r.iterations, bool(r.converged)) for r in reps], off, info


# ---- 1. a consistent b ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,weighted,mode", CASES)
def test_consistent_b_follows_the_model(W, H, weighted, mode):
    device_solves(W, H, weighted, mode, 1)


@pytest.mark.parametrize("W,H,mode", CASES3)
def test_three_channels_stop_at_their_own_iterations(W, H, mode):
    device_solves(W, H, True, mode, 3)
    counts = [r[1] for r in model(W, H, True, mode, 3)[7]]
    if W * H > 100:
        assert len(set(counts)) == 3, counts                     # the scales of b do separate the channels


# ---- 2. b + 1e-3: the solve the default loop cannot make ----------------------------------------------------------------
@pytest.mark.parametrize("W,H,weighted,mode,Cn", [c + (1,) for c in CASES] + [(W, H, True, mode, 3) for W, H, mode in CASES3])
def test_inconsistent_b_converges_to_the_same_x(W, H, weighted, mode, Cn):
    good, reps, off, info = device_solves(W, H, weighted, mode, Cn)
    want = model(W, H, weighted, mode, Cn)[8]
    for c in range(Cn):
        n, conv = reps[c]
        assert np.all(np.isfinite(off[c])), c
        assert conv and want[c][2], (c, n)
        assert n == want[c][1], (c, n, want[c][1])
        err, ok = close_to_model(off[c], good[c])
        print(f"{W}x{H} {mode} channel {c}: {n} iterations, |x - x of the consistent b| {err:.3e}, mean(b) - 1e-3 = {info[c][0] - 1e-3:.3e}")
        assert ok, (c, err)
        shifted = model(W, H, weighted, mode, Cn)[3][c] + 1e-3
        assert abs(info[c][0] - exact_mean(shifted)) <= mean_bound(shifted), info[c]
        if c == 0:                                                   # (the unscaled b: its own sum is rounding alone)
            assert abs(info[c][0] - 1e-3) <= 1e-12, info[c]
        assert info[c][2] == W * H
        assert abs(info[c][1] - exact_mean(off[c])) <= mean_bound(off[c]), info[c]


# ---- 3. one V-cycle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,mode", [(W, H, mode) for W, H in SHAPES for mode in MODES if mode != "line" or nh.line_served(W, H)])
def test_apply_is_the_projected_vcycle(W, H, mode):
    levels, wx, wy, _, _, _, M, _, _ = model(W, H, True, mode, 1)
    # integers: sum(b), and with it mean(b) and b - mean(b), have the same bits in any order of summation
    b = nh.rng(7 * W + H).integers(-50, 51, (H, W)).astype(np.float64)
    b[0, 0] += 3.0 - (b.sum() % 2)                                   # (a sum that is not 0)
    want, z, bm = nh.projected_vcycle(M, b)
    assert bm != 0.0
    g = handle(W, H, 1, mode, wx, wy)
    g.set_b(b, 0)
    g.fill_x(123.0)
    g.mg_apply(MODES[mode][3])
    got, b_after = g.get_x(0), g.get_b(0)
    g.close()
    assert np.array_equal(bits(b_after), bits(b))                    # b itself is not modified
    err = float(np.abs(got - want).max())
    bound = mean_bound(z)
    if mode == "line":                                               # the line solves' bits differ from the model's: its own test's rule
        bound += 16.0 * lh.deviation(levels, b - bm, 1, 1.0)[0] * float(np.abs(z).max())
    print(f"{W}x{H} {mode}: |x - (z - mean(z))| {err:.3e}, bound {bound:.3e}, |mean(x)| {abs(exact_mean(got)):.3e}")
    assert err <= bound, (err, bound)
    assert abs(exact_mean(got)) <= mean_bound(z)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def refused(g, bs, xs):
    """Both calls return UNSUPPORTED and leave x and b as they were."""
    load(g, bs, xs)
    rep = (capi.Report * g.C)()
    assert g.L.ccp_grid_mg_conjugate_gradient(g.h, 1e-10, 50, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply(g.h, 2) == UNSUPPORTED
    for c in range(g.C):
        assert np.array_equal(bits(g.get_x(c)), bits(xs[c])) and np.array_equal(bits(g.get_b(c)), bits(bs[c])), c


@pytest.mark.parametrize("what", ["lambda", "fixed", "zero_weight"])
def test_an_operator_that_is_not_floating_is_refused(what):
    W, H, mode = 64, 48, "rescaled"
    _, _, _, bs, x0, _, _, _, _ = model(W, H, False, mode, 1)
    lam = fixed = wx = None
    if what == "lambda":
        lam = np.zeros((H, W), np.float32)
        lam[H // 2, W // 3] = 1e-3
    elif what == "fixed":
        fixed = np.zeros((H, W), np.uint8)
        fixed[H // 2, W // 3] = 1
    else:
        wx = np.ones((H, W), np.float32)
        wx[H // 2, W // 3] = 0.0
    g = handle(W, H, 1, mode, wx, None, lam, fixed)
    refused(g, bs, x0)
    refused(g, bs, x0)                                               # (the verdict is kept, not taken again)
    g.set_weights()                                                  # repaired: the census runs on the new operator
    check_consistent(g, W, H, False, mode, 1, "repaired: ")
    g.close()


@pytest.mark.parametrize("W,H", [(33, 1), (1, 33), (129, 2), (2, 129), (66, 2), (257, 3), (2048, 32)])
def test_line_smoother_with_a_one_row_level_is_refused(W, H):
    """A line-smoothed level of one row or column (level 0 at 33x1; level 1, 65x1, at 129x2; level 2 at 257x3; level 5,
    64x1, at 2048x32): its one line along the canvas is the singular operator itself (no neighbour across, no lambda; the
    coarse operators of a floating operator are floating), and an exact line solve of it divides by zero -- the model's
    Thomas solve does, tests/line_helpers.py -- so the mode refuses the pair, and solves the canvas with the point
    smoother."""
    assert not nh.line_served(W, H)
    wx, wy = nh.weights(W, H, 5)
    b = wh.rhs(nh.hierarchy("rescaled", W, H, wx, wy)[0], *nh.guidance(W, H, 6))
    x0 = nh.rng(8).uniform(0.0, 255.0, (H, W))
    g = handle(W, H, 1, "line", wx, wy)
    refused(g, [b], [x0])
    g.mg_set_smoother("point")
    load(g, [b], [x0])
    rep = g.mg_conjugate_gradient(1e-10 * float(np.linalg.norm(b)), 100)[0]
    assert rep.converged and np.all(np.isfinite(g.get_x(0)))
    g.close()


def test_batched_channels_are_refused():
    W, H, mode = 64, 48, "rescaled"
    _, wx, wy, bs, x0, _, _, _, _ = model(W, H, True, mode, 3)
    g = handle(W, H, 3, mode, wx, wy)
    g.mg_set_channels("batched")
    refused(g, bs, x0)
    g.mg_set_channels("sequential")
    check_consistent(g, W, H, True, mode, 3, "sequential again: ")
    g.close()


def test_one_channel_that_is_not_floating_refuses_the_handle():
    W, H, mode = 64, 48, "rescaled"
    dev = torch.device("cuda", 0)
    _, wx, wy, bs, x0, _, _, _, _ = model(W, H, True, mode, 3)
    g = handle(W, H, 3, mode)
    t = [torch.from_numpy(np.repeat(a[..., None], 3, axis=2)).to(dev) for a in (wx, wy)]
    lam = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    lam[H // 2, W // 3, 1] = 1e-3
    g.set_weights_per_channel_tensor(t[0], t[1], lam)
    refused(g, bs, x0)
    g.set_weights_per_channel_tensor(t[0], t[1], torch.zeros_like(lam))
    check_consistent(g, W, H, True, mode, 3, "per channel, repaired: ")
    g.close()


def test_setter_getter_and_info_at_the_boundary():
    W, H = 24, 16
    g = capi.Grid(W, H, 2, weighted=True)
    assert g.mg_get_nullspace() == "none"
    assert g.L.ccp_grid_mg_set_nullspace(g.h, 2) == BAD_ARG and g.L.ccp_grid_mg_set_nullspace(g.h, -1) == BAD_ARG
    g.mg_set_nullspace("constant")
    g.mg_set_nullspace(capi.MG_NULLSPACES["constant"])               # the current value: nothing happens
    assert g.mg_get_nullspace() == "constant"
    g.set_weights()                                                  # the value survives a new operator and the other setters
    g.mg_set_hierarchy("rescaled")
    g.mg_set_smoother("line")
    g.mg_set_smoother("point")
    assert g.mg_get_nullspace() == "constant"
    assert g.L.ccp_grid_mg_nullspace_info(g.h, 0, None, None, None) == STATE
    assert g.L.ccp_grid_mg_nullspace_info(g.h, 2, None, None, None) == BAD_ARG
    assert g.L.ccp_grid_mg_nullspace_info(g.h, -1, None, None, None) == BAD_ARG
    rep = (capi.Report * 2)()
    assert g.L.ccp_grid_mg_conjugate_gradient_rowblocked(g.h, 1e-10, 10, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply_rowblocked(g.h, 2) == UNSUPPORTED
    g.close()
    for plain in (capi.Grid(W, H, 1), capi.Grid(W, H, 1, mask=np.ones((H, W), np.uint8))):
        value = C.c_int32(-1)
        assert plain.L.ccp_grid_mg_set_nullspace(plain.h, 1) == UNSUPPORTED
        assert plain.L.ccp_grid_mg_set_nullspace(plain.h, 7) == BAD_ARG
        assert plain.L.ccp_grid_mg_get_nullspace(plain.h, C.byref(value)) == 0 and value.value == 0
        assert plain.L.ccp_grid_mg_nullspace_info(plain.h, 0, None, None, None) == UNSUPPORTED
        plain.close()


# ---- 5. the default is untouched ------------------------------------------------------------------------------------------
def test_round_trip_keeps_the_defaults_bits():
    W, H, mode = 257, 131, "rescaled"
    _, wx, wy, bs, x0, eps, _, _, _ = model(W, H, True, mode, 1)
    g = handle(W, H, 1, mode, wx, wy)
    load(g, bs, x0)
    assert g.mg_conjugate_gradient(eps, 100)[0].converged
    g.mg_apply(2)
    g.mg_set_nullspace("none")
    assert g.mg_get_nullspace() == "none"
    ref = capi.Grid(W, H, 1, weighted=True)
    ref.mg_set_hierarchy("rescaled")
    lam = np.full((H, W), 0.05, np.float32)
    fixed = (nh.rng(3).uniform(size=(H, W)) < 0.02).astype(np.uint8)
    gx, gy = (a[..., None] for a in nh.guidance(W, H, 5))
    f = nh.rng(6).uniform(0.0, 255.0, (H, W, 1)).astype(np.float32)
    for name in ("screened", "constrained"):
        out = []
        for x in (g, ref):
            if name == "screened":
                x.set_weights(wx, wy, lam)
                x.assemble_weighted_rhs(gx, gy, f, init_x=True)
            else:
                x.set_weights(wx, wy, None, fixed=fixed)
                x.assemble_constrained_rhs(gx, gy, f, f, init_x=True)
            tol = 1e-10 * float(np.linalg.norm(x.get_b(0)))
            rep = x.mg_conjugate_gradient(tol, 200)[0]
            out.append((x.get_x(0), rep.iterations, rep.converged, rep.last_l1_step))
        (xa, na, ca, la), (xb, nb, cb, lb) = out
        assert ca and cb, name
        assert na == nb and la == lb, (name, na, nb, la, lb)
        assert np.array_equal(bits(xa), bits(xb)), name
    g.close()
    ref.close()


# ---- 6. one operator per channel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(257, 131), (33, 1)])
def test_per_channel_operators_equal_one_channel_handles(W, H):
    dev = torch.device("cuda", 0)
    mode, Cn = "rescaled", 3
    ws = [nh.weights(W, H, 200 + c) for c in range(Cn)]
    gs = [nh.guidance(W, H, 300 + c) for c in range(Cn)]
    x0 = [nh.rng(400 + c).uniform(0.0, 255.0, (H, W)) for c in range(Cn)]
    bs = [wh.rhs(nh.hierarchy("rescaled", W, H, *ws[c])[0], *gs[c]) + 1e-3 for c in range(Cn)]
    eps = 1e-10 * float(np.linalg.norm(bs[0]))
    g = handle(W, H, Cn, mode)
    g.set_weights_per_channel_tensor(*(torch.from_numpy(np.stack([w[i] for w in ws], axis=2)).to(dev) for i in range(2)))
    load(g, bs, x0)
    reps = g.mg_conjugate_gradient(eps, 100)
    for c in range(Cn):
        one = handle(W, H, 1, mode, *ws[c])
        load(one, [bs[c]], [x0[c]])
        rep = one.mg_conjugate_gradient(eps, 100)[0]
        assert rep.converged and reps[c].converged, c
        assert rep.iterations == reps[c].iterations and rep.last_l1_step == reps[c].last_l1_step, c
        assert np.array_equal(bits(one.get_x(0)), bits(g.get_x(c))), c
        assert one.mg_nullspace_info(0) == g.mg_nullspace_info(c), c
        one.close()
    g.close()


# ---- 7. tensor_ops ----------------------------------------------------------------------------------------------------------
def test_integrate_gradients_returns_the_image():
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 257, 131, 3
    dev = torch.device("cuda", 0)
    img = nh.rng(11).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    f = img.astype(np.float32)
    gx, gy = np.zeros_like(f), np.zeros_like(f)
    gx[:, :-1] = f[:, 1:] - f[:, :-1]                                # exact in float32
    gy[:-1] = f[1:] - f[:-1]
    means = [exact_mean(img[..., c]) for c in range(Cn)]
    u = tensor_ops.integrate_gradients(torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev), mean=torch.tensor(means, dtype=torch.float64))
    assert u.dtype == torch.float64 and tuple(u.shape) == (H, W, Cn) and u.is_cuda
    u = u.cpu().numpy()
    # the model's own error at the same epsilon, and the device held to it plus the model-vs-device tolerance
    levels = nh.hierarchy("galerkin", W, H)
    M = nh.preconditioner(levels, "galerkin")
    bs = [wh.rhs(levels[0], gx[..., c], gy[..., c]) for c in range(Cn)]
    eps = 1e-10 * max(float(np.linalg.norm(b)) for b in bs)
    for c in range(Cn):
        want = img[..., c].astype(np.float64)
        x, n, conv, _, _ = nh.pcg(levels[0], M, bs[c], eps, 200, np.full((H, W), means[c]))
        e = float(np.abs(x - want).max())
        got = float(np.abs(u[..., c] - want).max())
        bound = e + 1e-6 * float(np.abs(want).max())
        print(f"integrate_gradients channel {c}: model {n} iterations, |model - image| {e:.3e}, |device - image| {got:.3e}, bound {bound:.3e}")
        assert conv
        assert got <= bound, (c, got, bound)
        assert abs(exact_mean(u[..., c]) - means[c]) <= mean_bound(u[..., c])
    # a zero field: b = 0, the answer is the constant image, and no solve runs on a tolerance of 0
    flat = tensor_ops.integrate_gradients(torch.zeros((H, W, Cn), dtype=torch.float32, device=dev), None, mean=means)
    assert np.array_equal(flat.cpu().numpy(), np.broadcast_to(np.array(means), (H, W, Cn)))
    # the same call through weighted_solve, and the refusal of a system that is not floating
    w = tensor_ops.weighted_solve(torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev), torch.from_numpy(img).to(dev), 200,
                                  out_dtype=torch.float64, nullspace="constant")
    assert float(np.abs(w.cpu().numpy() - img).max()) <= 1e-6 * 255   # from x = the image itself: 0 iterations
    with pytest.raises(capi.CcpError) as e:
        tensor_ops.weighted_solve(torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev), torch.from_numpy(img).to(dev), 200,
                                  data_weight=0.05, nullspace="constant")
    assert e.value.status == UNSUPPORTED
