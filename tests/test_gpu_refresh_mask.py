"""GPU: ccp_grid_reserve_constraints and ccp_grid_refresh_constrained_device (include/ccp_gs.h, "Changing the fixed pixels
of a weighted operator by enqueue only").

The reference is always the existing path on a FRESH handle -- the matching setter with the weights and the mask,
ccp_grid_mg_prepare, then the same calls -- and equality is of bits (refresh_mask_helpers.everything): no tolerance
anywhere, since the refresh runs the setter's arithmetic and the build's own launches.

1. a reservation is invisible; 2. a refresh to (weights', mask B) equals a fresh handle, over every ordered pair of masks
and every mode; 3. a value refresh afterwards keeps B; 4. the counts; 5. the verdicts that stay on the device; 6. the
refusals on the host; 7. tensor_ops.WeightedSolver."""
import ctypes as C

import numpy as np
import pytest
import torch

import constrained_helpers as ch
from coursecomputationalphotography_amd import capi, tensor_ops
from refresh_mask_helpers import (CAP, KINDS, MASKS, assert_same, enqueue_bits, everything, handle, mask, mask_tensor, operator_bits,
                                  ubits)
from replay_helpers import DEV, PER_CHANNEL, SENTINEL, images, weights
from test_gpu_refresh import island

pytestmark = pytest.mark.gpu

BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
EPS = 1e-6
SHAPE = {kind: (70, 40, 2) for kind in KINDS}
SHAPE["floating"] = (64, 48, 1)


def w64(kind, W, H, Cn, seed):
    return [t.to(torch.float64) for t in weights(kind, W, H, Cn, seed)]


# ---- 1. a reservation is invisible ------------------------------------------------------------------------------------------
INVISIBLE = [(kind, *SHAPE[kind]) for kind in KINDS] + [("rescaled", 257, 131, 3), ("rescaled", 33, 1, 1), ("rescaled", 3, 2, 1),
                                                        ("rescaled", 1, 1, 1)]


@pytest.mark.parametrize("kind,W,H,Cn", INVISIBLE)
def test_a_reservation_is_invisible(kind, W, H, Cn):
    w, img = w64(kind, W, H, Cn, 31 * W + H), images(W, H, Cn, 5)
    plain = handle(kind, W, H, Cn, w, None, reserve=False)
    want = everything(plain, kind, img, w, None, EPS)
    plain.close()
    print(f"{kind} {W}x{H}x{Cn}: iterations {want['iterations']}")
    assert W * H <= 6 or (want["iterations"] > 0).all()
    zero = mask_tensor(kind, "empty", W, H, Cn)
    for what, fixed in (("reserved, no mask", None), ("reserved, an all-zero mask", zero)):
        g = handle(kind, W, H, Cn, w, fixed, reserve=True)
        assert_same(everything(g, kind, img, w, None, EPS), want, (kind, what))
        g.refresh_constrained_tensor(*w, fixed)                # the planes are there: the call is accepted, and changes nothing
        assert g.operator_status() == 0
        assert_same(everything(g, kind, img, w, None, EPS), want, (kind, what, "after a refresh to the same"))
        g.close()


def test_a_reservation_waits_for_the_next_setter():
    W, H, Cn = 64, 48, 1
    w = w64("rescaled", W, H, Cn, 3)
    g = handle("rescaled", W, H, Cn, w, None, reserve=False)
    before = operator_bits(g)
    g.reserve_constraints()                                    # the installed operator stays, and still has no planes
    assert_same(operator_bits(g), before, "reserve")
    with pytest.raises(capi.CcpError) as err:
        g.refresh_constrained_tensor(*w, mask_tensor("rescaled", "ellipse", W, H, Cn))
    assert err.value.status == STATE
    g.set_weights_tensor(*w)
    g.mg_prepare(0)
    g.refresh_constrained_tensor(*w, mask_tensor("rescaled", "ellipse", W, H, Cn))
    assert g.constraint_info()[0] == int(mask("ellipse", W, H).sum())
    g.reserve_constraints(False)                               # and off again at the next setter
    g.set_weights_tensor(*w)
    g.mg_prepare(0)
    with pytest.raises(capi.CcpError) as err:
        g.refresh_constrained_tensor(*w, None)
    assert err.value.status == STATE
    assert_same(operator_bits(g), before, "unreserved again")
    g.close()


# ---- 2. a refresh equals a fresh handle -------------------------------------------------------------------------------------
class Fresh:
    """everything() of a fresh reserved handle set with (weights seed, mask), formed once per pair"""

    def __init__(self, kind, W, H, Cn, img, cap, full):
        self.kind, self.shape, self.img, self.cap, self.full, self.known = kind, (W, H, Cn), img, cap, full, {}

    def weights(self, seed):
        return w64(self.kind, *self.shape, seed)

    def __call__(self, seed, name):
        if (seed, name) not in self.known:
            w, fixed = self.weights(seed), mask_tensor(self.kind, name, *self.shape)
            g = handle(self.kind, *self.shape, w, fixed, reserve=True)
            self.known[seed, name] = everything(g, self.kind, self.img, w, fixed, EPS, self.cap, self.full)
            g.close()
        return self.known[seed, name]


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "floating"])
def test_every_ordered_pair_of_masks(kind):
    """A -> B for every A and B (A = B too), the weights changing with the mask: the operator, b, x and the report"""
    W, H, Cn = SHAPE[kind]
    img = images(W, H, Cn, 6)
    fresh = Fresh(kind, W, H, Cn, img, 12, False)
    g = handle(kind, W, H, Cn, fresh.weights(100), mask_tensor(kind, "ellipse", W, H, Cn), reserve=True)
    for i, a in enumerate(MASKS):
        for j, b in enumerate(MASKS):
            sa, sb = 100 + (i + j) % 2, 101 + (i + j) % 2
            g.refresh_constrained_tensor(*fresh.weights(sa), mask_tensor(kind, a, W, H, Cn))
            enqueue_bits(g, img, EPS, 3)                       # (the work vectors are not fresh either)
            w, fixed = fresh.weights(sb), mask_tensor(kind, b, W, H, Cn)
            g.refresh_constrained_tensor(*w, fixed)
            assert g.operator_status() == 0
            want = fresh(sb, b)
            assert_same(everything(g, kind, img, w, fixed, EPS, 12, False), want, (kind, a, "->", b))
            if a != b:                                         # and the check is not vacuous: B's solution is not A's
                assert not np.array_equal(want["x enqueue"], fresh(sb, a)["x enqueue"]), (kind, a, b)
    g.close()


CHAINS = [(kind, 257, 131, 3) for kind in KINDS if kind != "floating"] + [("rescaled", 33, 1, 1), ("rescaled", 3, 2, 1), ("rescaled", 1, 1, 1)]


@pytest.mark.parametrize("kind,W,H,Cn", CHAINS)
def test_a_chain_of_refreshes_equals_fresh_handles_in_every_call(kind, W, H, Cn):
    """installed WITHOUT a reservation with mask A (the planes exist: A fixes a pixel); then A -> B, -> empty -> B,
    -> full -> A, and a value refresh that keeps the set: every call of the postcondition, the counts included"""
    img = images(W, H, Cn, 7)
    fresh = Fresh(kind, W, H, Cn, img, CAP, True)
    g = handle(kind, W, H, Cn, fresh.weights(200), mask_tensor(kind, "border", W, H, Cn), reserve=False)
    steps = [(201, "holes"), (202, "empty"), (203, "holes"), (201, "full"), (200, "border")]
    prev = None
    for seed, name in steps:
        w, fixed = fresh.weights(seed), mask_tensor(kind, name, W, H, Cn)
        g.refresh_constrained_tensor(*w, fixed)
        assert g.operator_status() == 0
        want = fresh(seed, name)
        assert_same(everything(g, kind, img, w, fixed, EPS), want, (kind, W, H, seed, name))
        if prev is not None and min(W, H) > 2:                 # (on the tail-only canvases several of the masks coincide)
            assert not np.array_equal(want["x enqueue"], fresh(*prev)["x enqueue"]), (kind, name)
        prev = (seed, name)
        # 3. a value refresh afterwards keeps the new set: it reads the marks the constrained refresh wrote
        w2 = fresh.weights(seed + 10)
        g.refresh_weights_tensor(*w2)
        assert g.operator_status() == 0
        assert_same(everything(g, kind, img, w2, fixed, EPS), fresh(seed + 10, name), (kind, W, H, name, "then a value refresh"))
    g.close()


def test_floating_operator_is_refreshed_with_the_empty_set():
    kind, (W, H, Cn) = "floating", SHAPE["floating"]
    img = images(W, H, Cn, 8)
    fresh = Fresh(kind, W, H, Cn, img, 100, True)
    g = handle(kind, W, H, Cn, fresh.weights(300), None, reserve=True)
    for seed, fixed in ((301, None), (302, mask_tensor(kind, "empty", W, H, Cn))):
        w = fresh.weights(seed)
        g.refresh_constrained_tensor(*w, fixed)
        assert g.operator_status() == 0
        assert_same(everything(g, kind, img, w, fixed, EPS, 100), fresh(seed, "empty"), (kind, seed))
    g.close()


# ---- 4. the counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,H,Cn", [("rescaled", 70, 40, 2), ("per_channel", 70, 40, 3), ("rescaled", 257, 131, 1)])
def test_counts_follow_every_refresh(kind, W, H, Cn):
    def expected(w, fixed, c):
        pick = (lambda t: t[..., c]) if kind in PER_CHANNEL else (lambda t: t)
        wx, wy, lam, fx = (pick(t).cpu().numpy() for t in (*w, fixed))
        return ch.counts(ch.level0(W, H, wx.astype(np.float64), wy.astype(np.float64), lam.astype(np.float64), fx))

    w0 = w64(kind, W, H, Cn, 400)
    g = handle(kind, W, H, Cn, w0, None, reserve=True)
    for k, name in enumerate(MASKS + ("holes", "empty")):
        w = w64(kind, W, H, Cn, 401 + k)
        island(w, 5, 9, 7, 12)                                  # dead free pixels, partly under the masks
        island(w, H // 2, H // 2 + 2, W // 2, W // 2 + 3)
        fixed = mask_tensor(kind, name, W, H, Cn)
        g.refresh_constrained_tensor(*w, fixed)
        got, want = [g.constraint_info(c) for c in range(Cn)], [expected(w, fixed, c) for c in range(Cn)]
        assert got == want, (kind, name, got, want)
        w2 = w64(kind, W, H, Cn, 450 + k)                       # no island: the dead count changes, the fixed count must stay
        g.refresh_weights_tensor(*w2)
        got, want = [g.constraint_info(c) for c in range(Cn)], [expected(w2, fixed, c) for c in range(Cn)]
        assert got == want, (kind, name, "after a value refresh", got, want)
    fixed = mask_tensor(kind, "block", W, H, Cn)               # a setter invalidates the device's fixed counts: its own hold
    if kind in PER_CHANNEL:
        g.set_weights_per_channel_tensor(*w0, fixed=fixed)
    else:
        g.set_weights_tensor(*w0, fixed=fixed)
    assert [g.constraint_info(c) for c in range(Cn)] == [expected(w0, fixed, c) for c in range(Cn)]
    g.mg_prepare(0)
    g.refresh_weights_tensor(*w0)
    assert [g.constraint_info(c) for c in range(Cn)] == [expected(w0, fixed, c) for c in range(Cn)]
    g.close()


# ---- 5. verdicts that stay on the device ------------------------------------------------------------------------------------
def snapshot(g):
    return ubits(g.get_x_tensor()), ubits(g.get_b_tensor())


def refused_on_the_device(g, kind, img, bad, fixed, status, what):
    enqueue_bits(g, img, EPS, 5)                               # a good right-hand side and some x
    g.refresh_constrained_tensor(*bad, fixed)                  # returns CCP_OK: the verdict stays on the device
    before = snapshot(g)
    report = torch.full((g.C, 6), SENTINEL, dtype=torch.float64, device=DEV)
    g.mg_conjugate_gradient_enqueue(EPS, 20, 0, report)
    torch.cuda.synchronize()
    for a, b in zip(snapshot(g), before):
        assert np.array_equal(a, b), (what, "the enqueue solve moved x or b")
    rep = report.cpu().numpy()
    assert (rep[:, 0] == 0).all() and (rep[:, 1] == 0).all() and (rep[:, 5] == float(status)).all(), (what, rep)
    assert g.operator_status() == status, what


@pytest.mark.parametrize("trigger,kind,status", [("nan_at_fixed", "rescaled", 1), ("negative_lambda_at_free", "per_channel", 1),
                                                 ("f32_range", "f32", 2)])
def test_refusals_on_the_device(trigger, kind, status):
    W, H, Cn = 70, 40, 2
    img = images(W, H, Cn, 9)
    fresh = Fresh(kind, W, H, Cn, img, CAP, True)
    g = handle(kind, W, H, Cn, fresh.weights(500), mask_tensor(kind, "ellipse", W, H, Cn), reserve=True)
    fixed = mask_tensor(kind, "block", W, H, Cn)
    plane = fixed if fixed.dim() == 2 else fixed[..., 0]
    bad = fresh.weights(501)
    at = lambda t: t if t.dim() == 2 else t[..., 0]
    if trigger == "nan_at_fixed":                              # every weight is checked, those of fixed pixels too
        assert int(plane[30, 60]) == 1
        at(bad[0])[30, 60] = float("nan")
    elif trigger == "negative_lambda_at_free":
        assert int(plane[10, 10]) == 0
        at(bad[2])[10, 10] = -0.5
    else:
        at(bad[1])[7, 9] = 1e39
    refused_on_the_device(g, kind, img, bad, fixed, status, trigger)
    marks = torch.stack([torch.from_numpy(np.asarray(g.mg_level(0, c)[0])) for c in range(Cn)], dim=-1)
    want_dead = fixed if fixed.dim() == 3 else fixed.unsqueeze(-1).expand(H, W, Cn)
    assert bool(((marks == 0) | (want_dead.cpu() == 0)).all()), "a fixed pixel of the new mask has a live row"
    # poisoned, not dropped: a good refresh of either kind restores the operator, with the NEW marks
    w = fresh.weights(502)
    g.refresh_weights_tensor(*w)
    assert g.operator_status() == 0
    assert_same(everything(g, kind, img, w, fixed, EPS), fresh(502, "block"), (trigger, "a value refresh after it"))
    g.refresh_constrained_tensor(*bad, fixed)
    assert g.operator_status() == status
    w, fixed = fresh.weights(503), mask_tensor(kind, "anchors", W, H, Cn)
    g.refresh_constrained_tensor(*w, fixed)
    assert g.operator_status() == 0
    assert_same(everything(g, kind, img, w, fixed, EPS), fresh(503, "anchors"), (trigger, "a constrained refresh after it"))
    g.close()


def test_a_fixed_pixel_is_not_floating():
    kind, (W, H, Cn) = "floating", SHAPE["floating"]
    img = images(W, H, Cn, 10)
    fresh = Fresh(kind, W, H, Cn, img, 100, True)
    g = handle(kind, W, H, Cn, fresh.weights(600), None, reserve=True)
    for k, name in enumerate(("anchors", "empty", "ellipse", "empty")):       # one handle, back and forth
        w, fixed = fresh.weights(601 + k), mask_tensor(kind, name, W, H, Cn)
        if name == "empty":
            g.refresh_constrained_tensor(*w, fixed if k == 1 else None)
            assert g.operator_status() == 0
            assert_same(everything(g, kind, img, w, None, EPS, 100), fresh(601 + k, "empty"), (kind, k))
        else:
            refused_on_the_device(g, kind, img, w, fixed, 4, name)
            assert g.constraint_info()[0] == int(mask(name, W, H).sum())
    g.close()


# ---- 6. refusals on the host: nothing is enqueued ---------------------------------------------------------------------------
def refused(g, status, w, fixed):
    before = snapshot(g)
    with pytest.raises(capi.CcpError) as err:
        g.refresh_constrained_tensor(*w, fixed)
    torch.cuda.synchronize()
    assert err.value.status == status
    for a, b in zip(snapshot(g), before):
        assert np.array_equal(a, b)


def test_refusals_on_the_host():
    kind, W, H, Cn = "rescaled", 64, 48, 2
    w, fixed = w64(kind, W, H, Cn, 71), mask_tensor(kind, "ellipse", W, H, Cn)
    g = capi.Grid(W, H, Cn, weighted=True)
    g.reserve_constraints()
    refused(g, STATE, w, fixed)                                # no operator installed
    g.close()
    for how in (None, mask_tensor(kind, "empty", W, H, Cn)):   # unreserved, installed without a fixed pixel: no planes
        g = handle(kind, W, H, Cn, w, how, reserve=False)
        levels = operator_bits(g)
        refused(g, STATE, w, fixed)
        refused(g, STATE, w, None)
        assert_same(operator_bits(g), levels, "no planes")
        g.refresh_weights_tensor(*w)                           # (the value refresh needs none)
        g.close()
    g = handle(kind, W, H, Cn, w, fixed, reserve=True, prepare=False)
    refused(g, STATE, w, fixed)                                # not prepared
    g.mg_prepare(0)
    levels = operator_bits(g)
    g.mg_set_precision("f32")
    refused(g, STATE, w, fixed)                                # a mode setter since prepare
    g.mg_set_precision("f64")
    g.mg_prepare(0)
    g.mg_set_nullspace("constant")
    refused(g, STATE, w, fixed)                                # ... one that frees nothing, too
    g.mg_set_nullspace("none")
    with pytest.raises(ValueError):                            # H x W x C views on a shared operator
        g.refresh_constrained_tensor(*w, mask_tensor("per_channel", "ellipse", W, H, Cn))
    before = snapshot(g)
    view = lambda t, dtype, ptr=True: C.byref(capi.DeviceArray(t.data_ptr() if ptr else None, dtype, 0, 0, W, 1, 0))
    call = g.L.ccp_grid_refresh_constrained_device
    assert call(g.h, view(w[0], capi.DTYPE_U8), None, None, None) == BAD_ARG                       # a weight's dtype
    assert call(g.h, None, None, None, view(fixed, capi.DTYPE_F64, ptr=False)) == BAD_ARG           # a mask without data
    assert call(g.h, None, None, None, view(fixed, 99)) == BAD_ARG                                  # a mask's dtype
    far = capi.DeviceArray(fixed.data_ptr(), capi.DTYPE_U8, 0, 0, 1 << 40, 1, 0)
    assert call(g.h, None, None, None, C.byref(far)) == BAD_ARG                                     # H rows do not fit the allocation
    with pytest.raises(ValueError):                                                                # wrong extents
        g.refresh_constrained_tensor(*w, fixed[:-1])
    torch.cuda.synchronize()
    for a, b in zip(snapshot(g), before):
        assert np.array_equal(a, b)
    assert_same(operator_bits(g), levels, "refused views")
    assert g.operator_status() == 0
    g.refresh_constrained_tensor(*w, fixed)                    # prepared and good: accepted
    assert g.operator_status() == 0
    g.close()
    s = capi.Grid(W, H, 1)                                     # a structured handle: the setters' status
    with pytest.raises(capi.CcpError) as err:
        s.refresh_constrained_tensor(w[0], w[1], w[2], fixed)
    assert err.value.status == UNSUPPORTED
    with pytest.raises(capi.CcpError) as err:
        s.reserve_constraints()
    assert err.value.status == UNSUPPORTED
    s.close()


# ---- 7. tensor_ops.WeightedSolver -------------------------------------------------------------------------------------------
def tbits(t):
    return t.detach().contiguous().view(torch.int64)


def test_refresh_constraints_equals_constrained_solve():
    kind, W, H, Cn = "rescaled", 257, 131, 3
    w0, w1 = w64(kind, W, H, Cn, 81), w64(kind, W, H, Cn, 82)
    a, b = mask_tensor(kind, "ellipse", W, H, Cn), mask_tensor(kind, "anchors", W, H, Cn)
    gx, gy, f, values = images(W, H, Cn, 8)
    eps, cap = 1e-6, 60
    # constrained_solve's own tolerance: both stop at sqrt(r'r) < eps, so each is within eps / lambda_min(A) of the
    # minimiser in the 2-norm; lambda_min >= the data weight 1e-2, hence 2 eps / 1e-2 bounds every pixel's difference
    want = tensor_ops.constrained_solve(gx, gy, f, values, b, cap, wx=w1[0], wy=w1[1], data_weight=w1[2], out_dtype=torch.float64, epsilon=eps,
                                        hierarchy="rescaled")
    with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=cap, epsilon=eps) as solver, \
            tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=cap, epsilon=eps) as fresh:
        with pytest.raises(RuntimeError):
            solver.refresh_constraints(*w1, b)                 # no operator yet
        solver.reserve_constraints()
        solver.set_operator(*w0, a)
        solver.solve(gx, gy, f, values, x0=f)
        solver.refresh_constraints(*w1, b)
        report = torch.full((Cn, 6), SENTINEL, dtype=torch.float64, device=DEV)
        got, _ = solver.solve(gx, gy, f, values, x0=f, report=report)
        fresh.set_operator(*w1, b)
        twin, _ = fresh.solve(gx, gy, f, values, x0=f)
        torch.cuda.synchronize()
        assert bool((report[:, 1] == 1.0).all()) and bool((report[:, 5] == 0.0).all()), report
        assert torch.equal(tbits(got), tbits(twin))
        err = float((got - want).abs().max())
        print(f"refresh_constraints against constrained_solve: max |difference| {err:.3e} (bound {2 * eps / 1e-2:.1e})")
        assert err <= 2 * eps / 1e-2


def test_two_forwards_on_two_masks_then_their_backwards():
    kind, W, H, Cn = "rescaled", 64, 48, 2
    ws = [w64(kind, W, H, Cn, seed) for seed in (91, 92, 93)]
    masks = [mask_tensor(kind, n, W, H, Cn) for n in ("ellipse", "block")]
    gx, gy, f, values = images(W, H, Cn, 9)
    loss_w = [images(W, H, Cn, 10 + k)[2] for k in range(2)]
    eps, cap = 1e-8, 60
    leaves = lambda: [t.clone().requires_grad_(True) for t in (gx, gy, f, values)]

    def alone(w, fixed, wgt):                                  # a solver that only ever held (w, fixed)
        with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=cap, epsilon=eps) as s:
            s.set_operator(*w, fixed)
            a = leaves()
            u, _ = s.solve_grad(*a, x0=f)
            (u * wgt).sum().backward()
            torch.cuda.synchronize()
            return u.detach(), [t.grad for t in a]

    refs = [alone(ws[1], masks[0], loss_w[0]), alone(ws[2], masks[1], loss_w[1])]
    assert not torch.equal(tbits(refs[0][0]), tbits(refs[1][0]))
    with tensor_ops.WeightedSolver(H, W, Cn, DEV, iterations=cap, epsilon=eps) as solver:
        solver.reserve_constraints()
        solver.set_operator(*ws[0], None)
        solver.refresh_constraints(*ws[1], masks[0])
        a1 = leaves()
        u1, _ = solver.solve_grad(*a1, x0=f)
        solver.refresh_constraints(*ws[2], masks[1])
        a2 = leaves()
        u2, _ = solver.solve_grad(*a2, x0=f)
        (u2 * loss_w[1]).sum().backward()                      # in reverse order: the handle holds mask 1, then needs mask 0 back
        (u1 * loss_w[0]).sum().backward()
        torch.cuda.synchronize()
        for (u, a), (u_ref, g_ref), what in (((u1, a1), refs[0], "first"), ((u2, a2), refs[1], "second")):
            assert torch.equal(tbits(u), tbits(u_ref)), what
            for t, r, name in zip(a, g_ref, ("gx", "gy", "f", "values")):
                assert t.grad is not None and t.grad.dtype == r.dtype and t.grad.shape == r.shape, (what, name)
                assert torch.equal(t.grad.contiguous().view(torch.uint8), r.contiguous().view(torch.uint8)), (what, name)
