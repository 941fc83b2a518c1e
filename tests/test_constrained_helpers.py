"""CPU: tests/constrained_helpers.py (the numpy model of weighted grid handles with fixed pixels) against first
principles: the constrained operator and b are the energy's derivatives with the fixed pixels substituted, d is lam' plus
the free couplings, an empty F gives weighted_helpers' bits, the V-cycle stays symmetric positive definite for both
hierarchy kinds, the PCG leaves fixed pixels alone; and the new ABI calls refuse without a device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as sla

import constrained_helpers as ch
import mg_helpers as mg
import test_weighted_helpers as twh
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 6), (33, 7), (17, 18)]      # (W, H)
KINDS = ("galerkin", "rescaled")


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def random_fixed(W, H, seed, share=0.3):
    return rng(seed).uniform(size=(H, W)) < share


def fields(W, H, seed, n=4):
    g = rng(seed)
    return [g.uniform(-50, 50, (H, W)).astype(np.float32) for _ in range(n)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_operator_and_rhs_are_the_energy_derivatives_with_fixed_pixels_substituted(W, H):
    wx, wy, lam = twh.random_weights(W, H, 10 + W * H)
    fixed = random_fixed(W, H, 3 + W)
    gx, gy, f, v = fields(W, H, 20 + W)
    lv = ch.level0(W, H, wx, wy, lam, fixed)
    A_ff, b_f, free = ch.free_system(W, H, wx, wy, lam, fixed, gx, gy, f, v)
    got = wh.matrix(lv).toarray()
    assert np.allclose(got[np.ix_(free, free)], A_ff.toarray(), rtol=1e-15, atol=1e-12)
    fix = np.flatnonzero(fixed.ravel())
    assert not got[fix].any() and not got[:, fix].any()                  # fixed pixels: empty rows and columns
    assert np.allclose(ch.rhs(lv, gx, gy, f, v).ravel()[free], b_f, rtol=1e-12, atol=1e-9)
    assert not ch.rhs(lv, gx, gy, f, v).ravel()[fix].any()
    # d = lam' + the free couplings, to rounding
    coupling = mg._shift(lv.ws, -1, 0) + mg._shift(lv.we, 0, -1) + lv.we + lv.ws
    assert np.allclose(lv.d, np.where(fixed, 0.0, lv.lam + coupling), rtol=1e-14, atol=1e-14)
    assert np.all(lv.lam >= 0) and not lv.lam[fixed].any()
    # we + ce, ws + cs: the original weights wherever an end is free
    full = wh.Level0(*wh.coefficients(W, H, wx, wy, lam))
    both_e = fixed & ch._shift_mask(fixed, 0, 1)
    both_s = fixed & ch._shift_mask(fixed, 1, 0)
    assert np.array_equal(lv.we + lv.ce, np.where(both_e, 0.0, full.we))
    assert np.array_equal(lv.ws + lv.cs, np.where(both_s, 0.0, full.ws))


@pytest.mark.parametrize("W,H", SHAPES)
def test_empty_f_is_bit_identical_to_weighted_helpers(W, H):
    wx, wy, lam = twh.random_weights(W, H, 40 + W)
    gx, gy, f, v = fields(W, H, 41 + W)
    for fixed in (None, np.zeros((H, W), np.uint8)):
        for kind, ref in (("galerkin", wh.hierarchy(W, H, wx, wy, lam)), ("rescaled", __import__("rescaled_helpers").hierarchy(W, H, wx, wy, lam))):
            got = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
            assert len(got) == len(ref)
            for a, b in zip(got, ref):
                for p, q in zip((a.d, a.we, a.ws, a.lam), (b.d, b.we, b.ws, b.lam)):
                    assert np.array_equal(p, q)
        lv = ch.level0(W, H, wx, wy, lam, fixed)
        assert np.array_equal(ch.rhs(lv, gx, gy, f, v), wh.rhs(wh.hierarchy(W, H, wx, wy, lam)[0], gx, gy, f))
        assert not lv.ce.any() and not lv.cs.any() and ch.counts(lv)[0] == 0 and ch.counts(lv)[2] == 0


def test_every_pixel_fixed_and_counts():
    W, H = 7, 5
    wx, wy, lam = twh.random_weights(W, H, 5, zeros=False)
    lv = ch.level0(W, H, wx, wy, lam, np.ones((H, W), np.uint8))
    assert not lv.d.any() and not lv.we.any() and not lv.ws.any() and not lv.lam.any() and not lv.ce.any() and not lv.cs.any()
    assert ch.counts(lv) == (W * H, 0, 0)
    one = np.zeros((H, W), np.uint8)
    one[2, 3] = 1
    assert ch.counts(ch.level0(W, H, wx, wy, lam, one)) == (1, W * H - 1, 4)
    v = rng(1).uniform(0, 9, (H, W))
    assert np.array_equal(ch.x_after(lv, np.full((H, W), 7.0), None, v, init=True), v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", [(8, 8), (13, 10)])
def test_vcycle_is_spd_on_constrained_operators(W, H, kind):
    import rescaled_helpers as rh
    pm = rh.preconditioner_matrix if kind == "rescaled" else wh.preconditioner_matrix
    fixed = random_fixed(W, H, W + H, 0.2)
    for name, wx, wy, lam in twh.operators(W, H):
        levels = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
        for nu in (1, 2):
            M, live = pm(levels, nu)
            assert not fixed.ravel()[live].any()
            scale = np.abs(M).max()
            assert np.allclose(M, M.T, rtol=0, atol=1e-12 * scale), f"{name} nu={nu}: not symmetric"
            ev = np.linalg.eigvalsh(0.5 * (M + M.T))
            assert ev.min() > 1e-10 * ev.max(), f"{name} nu={nu}: smallest eigenvalue {ev.min():.3e} of {ev.max():.3e}"


@pytest.mark.parametrize("kind", KINDS)
def test_pcg_solves_the_free_system_and_leaves_fixed_pixels_alone(kind):
    """Poisson (lam = 0) in a blob that reaches the canvas border, anchored by the fixed pixels around it."""
    W, H = 48, 40
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = ((xx - 10) / 30.0) ** 2 + ((yy - 20) / 14.0) ** 2 > 1.0      # the ellipse crosses x = 0
    gx, gy, f, v = fields(W, H, 77)
    levels = ch.hierarchy(W, H, None, None, None, fixed, kind)
    b = ch.rhs(levels[0], gx, gy, None, v)
    x0 = ch.x_after(levels[0], np.zeros((H, W)), None, v)
    x, it, conv, _ = ch.pcg(levels, b, 1e-10 * np.linalg.norm(b), 100, x0=x0, kind=kind)
    assert conv and it <= 20, (it, conv)
    assert np.array_equal(x[fixed], v.astype(np.float64)[fixed])
    A_ff, b_f, free = ch.free_system(W, H, None, None, None, fixed, gx, gy, None, v)
    want = sla.spsolve(A_ff.tocsc(), b_f)
    assert np.abs(x.ravel()[free] - want).max() <= 1e-6 * np.abs(want).max()


# ---- the ABI refuses without a device -----------------------------------------------------------------------------------
BAD_ARG = 1


def test_constrained_abi_refusals_without_a_device():
    """NULL handles are refused before any device is touched; the calls are exported with the declared names."""
    L = capi.load()
    assert L.ccp_grid_set_weights_constrained_host(None, None, None, None, 0, None, 0) == BAD_ARG
    assert L.ccp_grid_set_weights_constrained_device(None, None, None, None, None) == BAD_ARG
    assert L.ccp_grid_assemble_constrained_rhs(None, None, None, 0, None, 0, None, 0, 0) == BAD_ARG
    assert L.ccp_grid_assemble_constrained_rhs_device(None, None, None, None, None, 0) == BAD_ARG
    n = C.c_int64(-7)
    assert L.ccp_grid_constraint_info(None, C.byref(n), None, None) == BAD_ARG and n.value == -7
    assert L.ccp_abi_version() == 6
