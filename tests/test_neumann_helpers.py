"""CPU: the numpy model of CCP_MG_NULLSPACE_CONSTANT (tests/neumann_helpers.py) is a sound solver of the floating system.

P M P (P the mean-free projector, M one V-cycle) is symmetric positive semi-definite with exactly the constants as its
null space; the projected loop reproduces scipy's mean-pinned direct solve on unit and on random weights; it needs at
most one iteration more than the existing loop on a consistent b and no more at 257x131 than at 64x48; and a b that is
off by a constant, on which the existing loop does not converge, takes the projected loop as many iterations as the
consistent one."""
import functools

import numpy as np
import pytest

import neumann_helpers as nh

KINDS = ["galerkin", "rescaled"]


@functools.lru_cache(maxsize=None)
def system(kind, W, H, weighted):
    return nh.system(kind, W, H, weighted)


@functools.lru_cache(maxsize=None)
def solves(kind, W, H):
    """Unit weights, x0 = 0, epsilon = 1e-10 |b|: (the existing loop, the projected loop, the projected loop on b + 1e-3)."""
    levels, b = system(kind, W, H, False)[:2]
    eps = 1e-10 * float(np.linalg.norm(b))
    M = nh.preconditioner(levels, kind)
    plain = nh.plain_pcg(kind)(levels, b, eps, 100)
    proj = nh.pcg(levels[0], M, b, eps, 100)
    off = nh.pcg(levels[0], M, b + 1e-3, eps, 100)
    return plain, proj, off, eps


@pytest.mark.parametrize("kind", KINDS)
def test_projected_preconditioner_is_symmetric_psd_with_the_constants_as_null_space(kind):
    W, H = 16, 12
    n = W * H
    for weighted in (False, True):
        levels = system(kind, W, H, weighted)[0]
        B = nh.projected_preconditioner_matrix(levels, kind)
        scale = np.abs(B).max()
        assert np.abs(B - B.T).max() <= 1e-13 * scale
        ev = np.linalg.eigvalsh(0.5 * (B + B.T))
        assert abs(ev[0]) <= 1e-13 * ev[-1], ev[:3]              # one zero eigenvalue: the constants ...
        assert ev[1] > 1e-3 * ev[-1], ev[:3]                     # ... and nothing else near it
        assert np.abs(B @ np.ones(n)).max() <= 1e-13 * scale * n
        # and the operator itself: A 1 = 0
        assert np.abs(levels[0].apply(np.ones((H, W)))).max() <= 1e-13 * levels[0].d.max()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_projected_loop_reproduces_the_scipy_solve(kind, weighted):
    W, H = 64, 48
    levels, b = system(kind, W, H, weighted)[:2]
    x0 = nh.rng(9).uniform(0.0, 255.0, (H, W))
    eps = 1e-10 * float(np.linalg.norm(b))
    x, n, conv, norm, bm = nh.pcg(levels[0], nh.preconditioner(levels, kind), b, eps, 100, x0)
    assert conv and norm < eps, (n, norm)
    want, mu = nh.reference_solve(levels[0], b, nh.mean(x0))
    assert np.abs(x - want).max() <= 1e-6 * np.abs(want).max(), (n, float(np.abs(x - want).max()))
    assert abs(nh.mean(x) - nh.mean(x0)) <= 2 * W * H * 2.0 ** -53 * np.abs(x).max()
    assert abs(mu) <= 1e-9 and abs(bm) <= 1e-9                   # b = -div(w g) sums to zero up to rounding


@pytest.mark.parametrize("kind", KINDS)
def test_iteration_counts(kind):
    counts = {}
    for W, H in ((64, 48), (257, 131)):
        plain, proj, _, _ = solves(kind, W, H)
        assert plain[2] and proj[2], (W, H, plain[1], proj[1])
        assert proj[1] <= plain[1] + 1, (W, H, plain[1], proj[1])
        counts[W, H] = proj[1]
        print(f"{kind} {W}x{H}: existing loop {plain[1]}, projected loop {proj[1]}")
    assert counts[257, 131] <= counts[64, 48], counts


@pytest.mark.parametrize("W,H", [(64, 48), (257, 131)])
@pytest.mark.parametrize("kind", KINDS)
def test_inconsistent_b(kind, W, H):
    levels, b = system(kind, W, H, False)[:2]
    _, proj, off, eps = solves(kind, W, H)
    bad = nh.plain_pcg(kind)(levels, b + 1e-3, eps, 100)
    print(f"{kind} {W}x{H}: the existing loop on b + 1e-3: {bad[1]} iterations, converged {bad[2]}, max |x| {np.abs(bad[0]).max():.3e}")
    assert not bad[2] and bad[1] == 100
    assert off[2] and off[1] == proj[1], (off[1], proj[1])
    assert abs(off[4] - 1e-3) <= 1e-12
    assert np.abs(off[0] - proj[0]).max() <= 1e-9 * np.abs(proj[0]).max()
    assert abs(nh.mean(off[0])) <= 2 * W * H * 2.0 ** -53 * np.abs(off[0]).max()


@pytest.mark.parametrize("W,H", [(64, 2), (65, 33), (33, 1), (66, 2), (129, 2), (2, 129), (257, 3)])
def test_line_smoother_is_served_exactly_where_no_lined_level_has_one_row(W, H):
    """nh.line_served, the rule the library refuses by: the line V-cycle of a floating operator solves a singular line
    (and the Thomas solve divides by zero) exactly where a line-smoothed level has one row or one column; everywhere else
    the projected loop converges."""
    levels, b = nh.system("rescaled", W, H, True, seed=W + 3 * H)[:2]
    eps = 1e-10 * float(np.linalg.norm(b))
    with np.errstate(all="ignore"):
        x, n, conv, _, _ = nh.pcg(levels[0], nh.preconditioner(levels, "rescaled", 1, "f64", "line"), b, eps, 100)
    print(f"{W}x{H}: lined levels {nh.line_levels(W, H)}, {n} iterations, converged {conv}, finite {bool(np.all(np.isfinite(x)))}")
    if nh.line_served(W, H):
        assert conv and np.all(np.isfinite(x)), n
    else:
        assert not conv and not np.all(np.isfinite(x)), n
