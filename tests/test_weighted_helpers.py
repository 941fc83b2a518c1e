"""CPU: the weighted-grid helper behind test_gpu_weighted.py is sound, and the library refuses what a weighted handle
cannot do before it touches a device.

The helper's A is half the Hessian of E(u) = sum wx (Dx u - gx)^2 + sum wy (Dy u - gy)^2 + sum lam (u - f)^2, its b is
minus half the gradient of E at u = 0, its coarse levels are P^T A P (to rounding: real weights), SolveChannel's weights
reproduce the structured hierarchy of mg_helpers exactly, and its V-cycle (coarse correction scaled by 2) is a symmetric
positive definite preconditioner on screened (lam 1e-3, 1, 100), WLS (contrast down to 1e-4) and pure-data operators."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import mg_helpers as mg
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 6), (33, 7), (17, 18)]      # (W, H)


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def random_weights(W, H, seed, zeros=True):
    g = rng(seed)
    wx = g.uniform(0.0, 3.0, (H, W)).astype(np.float32)
    wy = g.uniform(0.0, 3.0, (H, W)).astype(np.float32)
    lam = g.uniform(0.0, 0.5, (H, W)).astype(np.float32)
    if zeros:
        wx[g.uniform(size=(H, W)) < 0.2] = 0
        wy[g.uniform(size=(H, W)) < 0.2] = 0
        lam[g.uniform(size=(H, W)) < 0.5] = 0
    return wx, wy, lam


def wls_weights(W, H, seed, contrast=1e-4):
    """Weights of an image with hard edges: 1 inside flat patches, `contrast` across their borders."""
    g = rng(seed)
    labels = (g.uniform(size=(H // 4 + 1, W // 4 + 1)) * 4).astype(int).repeat(4, 0).repeat(4, 1)[:H, :W]
    wx = np.ones((H, W), np.float32)
    wy = np.ones((H, W), np.float32)
    wx[:, :-1] = np.where(labels[:, 1:] != labels[:, :-1], contrast, 1.0)
    wy[:-1, :] = np.where(labels[1:, :] != labels[:-1, :], contrast, 1.0)
    return wx, wy, np.ones((H, W), np.float32)


def operators(W, H):
    yield "screened_1e-3", None, None, np.full((H, W), 1e-3, np.float32)
    yield "screened_1", None, None, np.ones((H, W), np.float32)
    yield "screened_100", None, None, np.full((H, W), 100.0, np.float32)
    yield ("wls_1e-4",) + wls_weights(W, H, 1, 1e-4)
    yield ("wls_1e-2",) + wls_weights(W, H, 2, 1e-2)
    yield "data_only", np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), rng(3).uniform(0.5, 2, (H, W)).astype(np.float32)
    yield ("random",) + random_weights(W, H, 4, zeros=False)


@pytest.mark.parametrize("W,H", SHAPES)
def test_operator_and_rhs_are_the_energy_derivatives(W, H):
    wx, wy, lam = random_weights(W, H, 10 + W * H)
    g = rng(20 + W)
    gx, gy, f = (g.uniform(-50, 50, (H, W)).astype(np.float32) for _ in range(3))
    lv = wh.hierarchy(W, H, wx, wy, lam)[0]
    Dx, Dy = wh.difference_matrices(W, H)
    Wx = sp.diags(wx[:, :-1].astype(np.float64).ravel())
    Wy = sp.diags(wy[:-1, :].astype(np.float64).ravel())
    L = sp.diags(lam.astype(np.float64).ravel())
    half_hessian = (Dx.T @ Wx @ Dx + Dy.T @ Wy @ Dy + L).toarray()
    assert np.allclose(wh.matrix(lv).toarray(), half_hessian, rtol=1e-15, atol=1e-12)
    minus_half_grad = Dx.T @ (Wx @ gx[:, :-1].astype(np.float64).ravel()) + Dy.T @ (Wy @ gy[:-1, :].astype(np.float64).ravel()) \
        + L @ f.astype(np.float64).ravel()
    assert np.allclose(wh.rhs(lv, gx, gy, f).ravel(), minus_half_grad, rtol=1e-12, atol=1e-9)
    z = g.uniform(-1, 1, (H, W))
    assert np.allclose(lv.apply(z).ravel(), half_hessian @ z.ravel(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("W,H", SHAPES)
def test_levels_are_galerkin(W, H):
    levels = wh.hierarchy(W, H, *random_weights(W, H, 30 + W))
    for k in range(len(levels) - 1):
        f, c = levels[k], levels[k + 1]
        Wc, Hc = (f.W + 1) // 2, (f.H + 1) // 2
        yy, xx = np.mgrid[0:f.H, 0:f.W]
        P = sp.csr_matrix((np.ones(f.W * f.H), (np.arange(f.W * f.H), ((yy // 2) * Wc + xx // 2).ravel())), shape=(f.W * f.H, Wc * Hc))
        galerkin = (P.T @ wh.matrix(f) @ P).toarray()
        assert np.allclose(wh.matrix(c).toarray(), galerkin, rtol=1e-13, atol=1e-12), f"level {k + 1}"
        assert np.all(c.d >= 0) and np.all(c.we >= 0) and np.all(c.ws >= 0) and np.all(c.lam >= 0)


@pytest.mark.parametrize("W,H", SHAPES + [(64, 64), (65, 31)])
def test_solve_channel_weights_give_the_structured_hierarchy(W, H):
    """Integer weights: both coarsenings are exact, so the weighted hierarchy IS the structured one."""
    got = wh.hierarchy(W, H, *wh.solve_channel_weights(W, H))
    want = mg.hierarchy(W, H)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a.coefficients(), b.coefficients()):
            assert np.array_equal(x, y), f"level {k}"
    g = rng(W * H)
    gx, gy = (g.uniform(-255, 255, (H, W)).astype(np.float32) for _ in range(2))
    f = np.zeros((H, W), np.float32)
    f[0, 0] = 17
    # SolveChannel's b (k_assemble_rhs order) from the same fields
    b = np.zeros((H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    cell = (xx < W - 1) & (yy < H - 1)
    gy64, gx64 = gy.astype(np.float64), gx.astype(np.float64)
    b = np.where((yy >= 1) & (xx < W - 1), b + 1.0 * mg._shift(gy64, -1, 0), b)
    b = np.where((xx >= 1) & (yy < H - 1), b + 1.0 * mg._shift(gx64, 0, -1), b)
    b = np.where(cell, b + -1.0 * gx64, b)
    b = np.where(cell, b + -1.0 * gy64, b)
    b[0, 0] += 1.0 * 17
    assert np.array_equal(wh.rhs(got[0], gx, gy, f), b)
    z = g.uniform(-100, 100, (H, W))
    assert np.array_equal(got[0].apply(z), want[0].apply(z))


@pytest.mark.parametrize("W,H", [(8, 8), (13, 10), (16, 16)])
def test_vcycle_is_spd_on_weighted_operators(W, H):
    """The coarse correction's scale 2.0 keeps M symmetric positive definite on every test operator."""
    for name, wx, wy, lam in operators(W, H):
        levels = wh.hierarchy(W, H, wx, wy, lam)
        for nu in (1, 2):
            M, _ = wh.preconditioner_matrix(levels, nu)
            scale = np.abs(M).max()
            assert np.allclose(M, M.T, rtol=0, atol=1e-12 * scale), f"{name} nu={nu}: not symmetric"
            ev = np.linalg.eigvalsh(0.5 * (M + M.T))
            assert ev.min() > 1e-10 * ev.max(), f"{name} nu={nu}: smallest eigenvalue {ev.min():.3e} of {ev.max():.3e}"


@pytest.mark.parametrize("name", ["screened_1e-3", "screened_100", "wls_1e-4", "data_only"])
def test_pcg_converges_fast(name):
    W, H = 48, 40
    wx, wy, lam = next((o[1:] for o in operators(W, H) if o[0] == name))
    levels = wh.hierarchy(W, H, wx, wy, lam)
    b = levels[0].apply(rng(5).uniform(0, 255, (H, W)))
    A = wh.matrix(levels[0]).tocsc()
    x, it, conv, _ = wh.pcg(levels, b, 1e-10 * np.linalg.norm(b), 200)
    assert conv and it <= 30, (it, conv)
    import scipy.sparse.linalg as sla
    assert np.allclose(x.ravel(), sla.spsolve(A, b.ravel()), rtol=0, atol=1e-6 * np.abs(b).max())


# ---- the ABI refuses without a device -----------------------------------------------------------------------------------
BAD_ARG, UNSUPPORTED = 1, 6


def test_weighted_abi_refusals_without_a_device():
    """NULL handles, and the flags a weighted grid cannot combine with, are refused before any device is touched."""
    L = capi.load()
    assert L.ccp_grid_set_weights_host(None, None, None, None, 0) == BAD_ARG
    assert L.ccp_grid_set_weights_device(None, None, None, None) == BAD_ARG
    assert L.ccp_grid_assemble_weighted_rhs(None, None, None, 0, None, 0, 0) == BAD_ARG
    assert L.ccp_grid_assemble_weighted_rhs_device(None, None, None, None, 0) == BAD_ARG
    h = C.c_void_p()
    for desc in (capi.GridDesc(8, 8, 1, 0, 8, 0, 0, capi.GRID_WEIGHTED | capi.GRID_DIRICHLET_MASK),
                 capi.GridDesc(8, 8, 1, 0, 4, 0, 0, capi.GRID_WEIGHTED),
                 capi.GridDesc(8, 8, 1, 2, 4, 1, 0, capi.GRID_WEIGHTED),
                 capi.GridDesc(8, 8, 1, 0, 8, 2, 0, capi.GRID_WEIGHTED)):
        assert L.ccp_grid_create(C.byref(desc), C.byref(h)) == UNSUPPORTED
        assert not h.value
