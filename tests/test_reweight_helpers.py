"""CPU: the numpy model of the reweighting pass (tests/reweight_helpers.py) against itself: the vectorised weights equal
the scalar triple loop bit for bit, the output conventions, the penalties' derivative, and the property the IRLS loop rests
on: with exact inner solves the energy never increases, for every penalty and coupling."""
import numpy as np
import pytest

import reweight_helpers as rh


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def inputs(W, H, C, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 255.0, (H, W, C))
    gx, gy = (rng.standard_normal((H, W, C)).astype(np.float32) for _ in range(2))
    bx, by = (rng.uniform(0.5, 2.0, (H, W)).astype(np.float32) for _ in range(2))
    return u, gx, gy, bx, by


@pytest.mark.parametrize("penalty,coupling", rh.PAIRS)
def test_weights_equal_the_scalar_loop(penalty, coupling):
    W, H, C = 5, 4, 2
    u, gx, gy, bx, by = inputs(W, H, C, 7)
    u[1, 2] = u[1, 3]                                          # a zero residual with zero guidance below
    for per_channel in (False, True):
        for g in ((gx, gy), (None, None)):
            for base in ((None, None), (bx, by)):
                got = rh.weights(u, g[0], g[1], penalty, coupling, 0.75, 1e-2, base[0], base[1], per_channel)
                want = rh.weights_scalar(u, g[0], g[1], penalty, coupling, 0.75, 1e-2, base[0], base[1], per_channel)
                for a, b in zip(got, want):
                    assert a.shape == ((H, W, C) if per_channel else (H, W))
                    assert np.array_equal(bits(a), bits(b)), (penalty, coupling, per_channel)


@pytest.mark.parametrize("penalty,coupling", rh.PAIRS)
def test_the_last_column_and_row_are_plus_zero(penalty, coupling):
    u, gx, gy, bx, by = inputs(5, 4, 2, 8)
    for per_channel in (False, True):
        wx, wy = rh.weights(u, gx, gy, penalty, coupling, 1.0, 1e-3, bx, by, per_channel)
        assert not bits(wx[:, -1]).any() and not bits(wy[-1]).any()      # +0.0: all bits clear
        assert (wx[:, :-1] > 0).all() and (wy[:-1] > 0).all()


def test_one_pixel_and_one_line():
    for W, H in ((1, 1), (7, 1), (1, 7)):
        u = np.random.default_rng(W).uniform(0, 1, (H, W, 2))
        for coupling in rh.COUPLINGS:
            wx, wy = rh.weights(u, None, None, "charbonnier", coupling, 1.0, 1e-2)
            assert wx.shape == (H, W) and not wx[:, -1].any() and not wy[-1].any()
            want = rh.weights_scalar(u, None, None, "charbonnier", coupling, 1.0, 1e-2)
            assert np.array_equal(bits(wx), bits(want[0])) and np.array_equal(bits(wy), bits(want[1]))


@pytest.mark.parametrize("penalty", rh.PENALTIES)
def test_psi_is_the_penalty_of_phi(penalty):
    """psi'(rho) = rho phi(rho^2), by central differences; psi is continuous where huber changes branch"""
    eps = 0.05
    rho = np.linspace(0.0, 0.4, 81)[1:] + 1.3e-3               # (off rho = eps, where huber's second derivative jumps)
    h = 1e-6
    assert abs(float(rh.psi(eps - 1e-12, penalty, eps)) - float(rh.psi(eps + 1e-12, penalty, eps))) < 1e-11
    slope = (rh.psi(rho + h, penalty, eps) - rh.psi(rho - h, penalty, eps)) / (2 * h)
    assert np.allclose(slope, rho * rh.phi(rho * rho, penalty, eps), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("penalty,coupling", rh.PAIRS)
def test_dense_irls_never_increases_the_energy(penalty, coupling):
    """12 x 9 x 2, a two-level step image plus seeded noise, strength 0.3, epsilon 1e-3, data weight 1, 8 outer steps"""
    f = rh.step_image(12, 9, 2, seed=5)
    iterates, E = rh.dense_irls(f, None, None, penalty, coupling, 0.3, 1e-3, 1.0, 8)
    steps = np.diff(E)
    print(f"{penalty} {coupling}: E {E[0]:.4f} -> {E[-1]:.4f}, largest step {steps.max():.3e}")
    assert len(iterates) == 8 and (steps <= 0.0).all(), (penalty, coupling, E)
    assert E[-1] < 0.75 * E[0]                                  # and it does denoise: well below E(f)


def test_true_residual_is_the_dense_systems():
    W, H, C = 6, 5, 2
    u, gx, gy, bx, by = inputs(W, H, C, 9)
    f = np.random.default_rng(1).uniform(0, 255, (H, W, C))
    wx, wy = rh.weights(u, gx, gy, "huber", "edge", 0.5, 1e-2, bx, by)
    rn, bn = rh.true_residual(u, wx, wy, 0.25, gx, gy, f)
    for c in range(C):
        A, b = rh.system(wx, wy, 0.25, gx[:, :, c].astype(np.float64), gy[:, :, c].astype(np.float64), f[:, :, c])
        assert np.isclose(bn[c], np.linalg.norm(b), rtol=1e-12)
        assert np.isclose(rn[c], np.linalg.norm(b - A @ u[:, :, c].ravel()), rtol=1e-10)
