"""CPU: the rescaled hierarchy of weighted handles (CCP_MG_HIERARCHY_RESCALED) in the numpy model of
tests/rescaled_helpers.py, and the two ABI calls that choose it.

The rescaled levels are the Galerkin levels of weighted_helpers with the edge weights scaled by 2^-k exactly and the same
lambda; the V-cycle with the unscaled correction is a symmetric positive definite preconditioner on the operators
test_weighted_helpers.py uses for the Galerkin cycle; and on screened systems the PCG count no longer grows with the image,
where the Galerkin hierarchy's does."""
import ctypes as C

import numpy as np
import pytest

import rescaled_helpers as rh
import test_weighted_helpers as twh
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

BAD_ARG = 1


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def dead_weights(W, H, seed):
    """Random float32 weights with zero edges, lambda = 0 areas and (where there is room) a dead pixel."""
    wx, wy, lam = twh.random_weights(W, H, seed)
    if W > 4 and H > 4:
        wx[2, 1:3] = 0
        wy[1:3, 2] = 0
        lam[2, 2] = 0
    return wx, wy, lam


# ---- 1. the relation between the two hierarchies ------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", twh.SHAPES + [(65, 31), (131, 77), (301, 203)])
def test_rescaled_levels_are_the_galerkin_levels_with_halved_edges(W, H):
    wx, wy, lam = dead_weights(W, H, 50 + W)
    legacy = wh.hierarchy(W, H, wx, wy, lam)
    levels = rh.hierarchy(W, H, wx, wy, lam)
    assert len(levels) == len(legacy)
    if W > 4 and H > 4:
        assert not legacy[0].live[2, 2]
    for k, (a, b) in enumerate(zip(levels, legacy)):
        assert np.array_equal(a.we, np.ldexp(b.we, -k)), f"level {k}: east weights"
        assert np.array_equal(a.ws, np.ldexp(b.ws, -k)), f"level {k}: south weights"
        assert np.array_equal(a.lam, b.lam), f"level {k}: lambda"
        # d = lam; += north; += west; += east; += south of the level's own (rescaled) weights
        d = a.lam.copy()
        d[1:, :] = d[1:, :] + a.ws[:-1, :]
        d[:, 1:] = d[:, 1:] + a.we[:, :-1]
        d = d + a.we
        d = d + a.ws
        assert np.array_equal(a.d, d), f"level {k}: diagonal"
        assert np.all(a.d >= 0) and np.all(a.we >= 0) and np.all(a.ws >= 0) and np.all(a.lam >= 0)
    for a, b in zip(levels[0].coefficients(), legacy[0].coefficients()):
        assert np.array_equal(a, b)


# ---- 2. the V-cycle is a symmetric positive definite preconditioner -----------------------------------------------------
@pytest.mark.parametrize("W,H", [(8, 8), (13, 10), (16, 16)])
def test_rescaled_vcycle_is_spd(W, H):
    for name, wx, wy, lam in twh.operators(W, H):
        levels = rh.hierarchy(W, H, wx, wy, lam)
        for nu in (1, 2):
            M, _ = rh.preconditioner_matrix(levels, nu)
            scale = np.abs(M).max()
            assert np.allclose(M, M.T, rtol=0, atol=1e-12 * scale), f"{name} nu={nu}: not symmetric"
            ev = np.linalg.eigvalsh(0.5 * (M + M.T))
            assert ev.min() > 1e-10 * ev.max(), f"{name} nu={nu}: smallest eigenvalue {ev.min():.3e} of {ev.max():.3e}"


# ---- 3. iteration counts, Galerkin against rescaled on the same system ---------------------------------------------------
def counts(W, H, wx, wy, lam, seed=5):
    """(Galerkin, rescaled) PCG iterations to 1e-10 |b| on b = A x, x uniform [0, 255), from x = 0, nu = 2."""
    legacy = wh.hierarchy(W, H, wx, wy, lam)
    levels = rh.hierarchy(W, H, wx, wy, lam)
    b = legacy[0].apply(rng(seed).uniform(0, 255, (H, W)))
    eps = 1e-10 * float(np.linalg.norm(b))
    _, il, cl, _ = wh.pcg(legacy, b, eps, 200)
    _, ir, cr, _ = rh.pcg(levels, b, eps, 200)
    assert cl and cr, (il, cl, ir, cr)
    return il, ir


def screened(W, H, lam):
    return None, None, np.full((H, W), lam, np.float32)


def test_screened_counts_stop_growing():
    l_small, r_small = counts(256, 192, *screened(256, 192, 1e-2))
    l_big, r_big = counts(509, 383, *screened(509, 383, 1e-2))
    print(f"screened 1e-2: 256x192 galerkin {l_small} rescaled {r_small}; 509x383 galerkin {l_big} rescaled {r_big}")
    assert 2 * r_big <= l_big, (l_big, r_big)
    assert r_big <= r_small + 2, (r_small, r_big)


def test_solve_channel_and_random_weights_are_no_worse():
    W, H = 509, 383
    il, ir = counts(W, H, *wh.solve_channel_weights(W, H))
    print(f"SolveChannel's weights 509x383: galerkin {il} rescaled {ir}")
    assert ir <= il + 1, (il, ir)
    g = rng(17)
    wx = g.uniform(0.1, 10.0, (H, W)).astype(np.float32)
    wy = g.uniform(0.1, 10.0, (H, W)).astype(np.float32)
    lam = np.where(g.uniform(size=(H, W)) < 0.01, 10.0, 0.0).astype(np.float32)
    il, ir = counts(W, H, wx, wy, lam)
    print(f"random weights 509x383: galerkin {il} rescaled {ir}")
    assert ir <= il + 1, (il, ir)


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------------
def test_hierarchy_calls_are_exported_and_refuse_without_a_device():
    L = capi.load()
    for name in ("ccp_grid_mg_set_hierarchy", "ccp_grid_mg_get_hierarchy"):
        assert hasattr(L, name), name
        assert name in capi.ABI_SYMBOLS, name
    kind = C.c_int32(7)
    assert L.ccp_grid_mg_set_hierarchy(None, capi.MG_HIERARCHY_RESCALED) == BAD_ARG
    assert L.ccp_grid_mg_set_hierarchy(None, 2) == BAD_ARG
    assert L.ccp_grid_mg_get_hierarchy(None, C.byref(kind)) == BAD_ARG
    assert L.ccp_grid_mg_get_hierarchy(None, None) == BAD_ARG
    assert kind.value == 7
    assert (capi.MG_HIERARCHY_GALERKIN, capi.MG_HIERARCHY_RESCALED) == (0, 1)
    assert capi.MG_HIERARCHIES == {"galerkin": 0, "rescaled": 1}
