"""CPU: the numpy model of the line V-cycle (tests/line_helpers.py) that tests/test_gpu_mg_line.py compares the device
with.  M^-1 is symmetric positive definite; the model's own iteration counts on the issue's cases (WLS smoothing of the
benchmark image at 188x142 and 376x283, sparse anchors at 188x142; rescaled hierarchy, nu = 1, to 1e-10 |b| from x = 0)
are pinned, as is their relation to the point smoother's; and the float64 model stays within a few ulps-times-depth of
the same model carried in np.longdouble on every GPU test shape -- the number the device tolerance is taken from.

The model's counts (this file asserts them), lines at nu = 1 against the point smoother at nu = 2:  WLS 188x142: 42
(point: 249);  WLS 376x283: 56 (point: 281);  anchors [8::32] at 188x142: 87 (point: not converged in 400);  anchors
[8::16] at 188x142: 43 (point: more than 86).  float64 model against the longdouble model, one V-cycle, max-norm relative
to max |z|: 7e-15 to 1.3e-13 over the shapes (257x131 the largest)."""
import functools

import numpy as np
import pytest

import line_helpers as lh
import rescaled_helpers as rh
import weighted_helpers as wh

# (case) -> the line model's iteration count, nu = 1, rescaled hierarchy
COUNTS = {"wls_188x142": 42, "wls_376x283": 56, "anchors32_188x142": 87, "anchors16_188x142": 43}
GPU_SHAPES = [(67, 3), (1, 40), (40, 1), (257, 131), (2053, 9), (9, 2053), (512, 384), (4099, 3), (8200, 2)]


@functools.lru_cache(maxsize=None)
def system(case):
    if case.startswith("wls_"):
        W, H = (int(v) for v in case[4:].split("x"))
        return lh.wls_system(W, H)
    step = int(case[7:9])
    return lh.anchor_system(188, 142, step)[:2]


@functools.lru_cache(maxsize=None)
def line_count(case):
    levels, b = system(case)
    eps = 1e-10 * float(np.linalg.norm(b))
    x, n, conv, norm = lh.pcg(levels, b, eps, 200, 1, 1.0)
    true = float(np.linalg.norm(b - levels[0].apply(x)))
    return n, conv, true, eps


@functools.lru_cache(maxsize=None)
def point_count(case, cap):
    levels, b = system(case)
    eps = 1e-10 * float(np.linalg.norm(b))
    _, n, conv, _ = rh.pcg(levels, b, eps, cap, 2)
    return n, conv


def small_operators():
    """The operators of test_weighted_helpers.py's preconditioner checks: unit weights, random weights, SolveChannel's."""
    W, H = 7, 5
    g = np.random.default_rng(11)
    wx, wy = (g.uniform(0.1, 10.0, (H, W)).astype(np.float32) for _ in range(2))
    lam = np.where(g.uniform(size=(H, W)) < 0.2, 1.0, 0.0).astype(np.float32)
    lam[0, 0] = 1.0
    yield "random", W, H, wx, wy, lam
    yield "solve_channel", W, H, *wh.solve_channel_weights(W, H)
    # wide enough for two line levels (70 -> 35 -> tail) and anisotropic
    W, H = 70, 6
    wx = g.uniform(10.0, 1000.0, (H, W)).astype(np.float32)
    wy = g.uniform(1e-3, 1e-1, (H, W)).astype(np.float32)
    yield "anisotropic", W, H, wx, wy, np.full((H, W), 0.01, np.float32)


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("kind", ["galerkin", "rescaled"])
def test_preconditioner_is_symmetric_positive_definite(kind, nu):
    for name, W, H, wx, wy, lam in small_operators():
        levels = (rh if kind == "rescaled" else wh).hierarchy(W, H, wx, wy, lam)
        M, live = lh.preconditioner_matrix(levels, nu, lh.CS[kind])
        scale = np.abs(M).max()
        # rounding only: 2.2e-16 x the condition of the line systems, which is <= (lambda + 4 w) / lambda = 4e5 on the
        # anisotropic operator
        assert np.abs(M - M.T).max() <= 1e-10 * scale, (name, kind, nu, np.abs(M - M.T).max() / scale)
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0, (name, kind, nu)


def test_line_solve_is_exact_and_dead_cells_split_the_line():
    g = np.random.default_rng(3)
    n, L = 41, 6
    w = g.uniform(1e-3, 1e3, (n, L))
    d = g.uniform(0.0, 1.0, (n, L)) + w + np.vstack([np.zeros((1, L)), w[:-1]])
    dead = np.zeros((n, L), bool)
    dead[[0, 9, 10, 12, 40], 1] = True                           # at both ends, adjacent, and a length-1 segment
    dead[:, 2] = True                                            # a wholly dead line
    w[dead] = 0.0
    w[:-1][dead[1:]] = 0.0
    d[dead] = 0.0
    rhs = g.normal(size=(n, L))
    x = lh._solve_lines(d, w, rhs)
    assert np.all(x[dead] == 0.0) and np.all(np.isfinite(x))
    wl = w.copy()
    wl[-1] = 0.0
    ax = d * x - wl * np.vstack([x[1:], np.zeros((1, L))]) - np.vstack([np.zeros((1, L)), wl[:-1] * x[:-1]])
    assert np.abs(np.where(dead, 0.0, ax - rhs)).max() <= 1e-9 * np.abs(rhs).max()


@pytest.mark.parametrize("case", sorted(COUNTS))
def test_iteration_counts_of_the_model(case):
    n, conv, true, eps = line_count(case)
    print(f"{case}: {n} iterations with lines, |b - A x| = {true:.3e}, epsilon = {eps:.3e}")
    assert conv and n == COUNTS[case], (case, n, conv)
    assert true <= 1.01 * eps, (case, true, eps)


@pytest.mark.parametrize("case", ["wls_188x142", "wls_376x283", "anchors16_188x142"])
def test_lines_need_at_most_half_the_point_smoothers_iterations(case):
    n, conv, _, _ = line_count(case)
    m, pconv = point_count(case, 2 * n + 1)                      # enough to decide: the point count must be >= 2 n
    print(f"{case}: lines {n}, point smoother {m}{'' if pconv else '+ (stopped)'}")
    assert conv and 2 * n <= m, (case, n, m)


def test_sparse_anchors_converge_with_lines_only():
    n, conv, _, _ = line_count("anchors32_188x142")
    assert conv and n <= 200, n
    m, pconv = point_count("anchors32_188x142", 400)
    assert not pconv and m == 400, (m, pconv)


@pytest.mark.parametrize("W,H", GPU_SHAPES)
def test_float64_model_against_the_extended_precision_model(W, H):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not wider than float64 here"
    worst = 0.0
    for kind in ("galerkin", "rescaled"):
        for nu in (1, 2):
            levels, b = lh.shape_system(W, H, kind)[:2]
            dev, _ = lh.deviation(levels, b, nu, lh.CS[kind])
            print(f"{W}x{H} {kind} nu={nu}: float64 model vs longdouble model {dev:.3e}")
            worst = max(worst, dev)
    assert 0.0 < worst < 1e-11, worst                            # the V-cycle is well conditioned: rounding, not growth


def test_float64_model_against_the_extended_precision_model_with_fixed_pixels():
    W, H = 257, 131
    for kind in ("galerkin", "rescaled"):
        levels, b = lh.shape_system(W, H, kind, fixed=True)[:2]
        dev, z = lh.deviation(levels, b, 1, lh.CS[kind])
        print(f"{W}x{H} fixed {kind}: float64 model vs longdouble model {dev:.3e}")
        assert np.all(z[~levels[0].live] == 0.0)
        assert 0.0 < dev < 1e-11, dev
