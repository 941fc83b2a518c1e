"""CPU: the numpy model of the backward pass (tests/adjoint_helpers.py) against central finite differences of the dense
solve.  L = sum G * u with a seeded G; every formula -- wx, wy, gx, gy, lambda, f, values -- must agree with
(L(p + h) - L(p - h)) / 2h, h = 1e-6, to 1e-7 of the gradient's largest entry (5e-9 was measured when the formulas were
derived; central differences of a smooth function carry O(h^2) = 1e-12 truncation and about 1e-16 / h = 1e-10 rounding,
times the system's conditioning).  Cases: 6 x 5 x 2 with about a quarter of the pixels fixed, no fixed pixels, every pixel
fixed, and dead pixels."""
import numpy as np
import pytest

import adjoint_helpers as ah
import constrained_helpers as ch

W, H, C = 6, 5, 2
STEP, BOUND = 1e-6, 1e-7


def problem(seed, fixed_share=0.25):
    r = np.random.default_rng(seed)
    p = dict(gx=r.uniform(-1, 1, (H, W, C)), gy=r.uniform(-1, 1, (H, W, C)), f=r.uniform(0, 1, (H, W, C)),
             wx=r.uniform(0.1, 10, (H, W)), wy=r.uniform(0.1, 10, (H, W)), lam=r.uniform(0.01, 1, (H, W)),
             values=r.uniform(0, 1, (H, W, C)))
    fixed = r.uniform(size=(H, W)) < fixed_share
    G = r.uniform(-1, 1, (H, W, C))
    return p, fixed, G


def loss(p, fixed, G):
    return float(np.sum(G * ah.dense_solve(fixed=fixed, shape=G.shape, **p)))


def central_differences(p, fixed, G, name, skip=None):
    out = np.zeros_like(p[name])
    for i in np.ndindex(out.shape):
        if skip is not None and skip[i[:2]]:
            continue
        q = {k: a.copy() for k, a in p.items()}
        q[name][i] += STEP
        up = loss(q, fixed, G)
        q[name][i] -= 2 * STEP
        out[i] = (up - loss(q, fixed, G)) / (2 * STEP)
    return out


def compare(p, fixed, G, skip=None):
    _, _, got = ah.dense_reference(G, fixed=fixed, **p)
    worst = {}
    for name in ah.PLANES + ah.IMAGES:
        sk = None if skip is None else skip.get(name)
        fd = central_differences(p, fixed, G, name, sk)
        g = got[name] if sk is None else np.where(sk if got[name].ndim == 2 else sk[..., None], 0.0, got[name])
        scale = max(np.abs(fd).max(), 1e-300)
        worst[name] = np.abs(g - fd).max() / scale
        assert worst[name] <= BOUND, (name, worst[name])
    print({k: f"{e:.2e}" for k, e in worst.items()})
    return got


def test_formulas_match_central_differences_with_fixed_pixels():
    p, fixed, G = problem(11)
    assert 0 < fixed.sum() < W * H
    got = compare(p, fixed, G)
    # what is zero by the formulas is +0.0
    for name in ("f", "lam"):
        z = got[name][fixed]
        assert np.all(z == 0.0) and not np.signbit(z).any()
    z = got["values"][~fixed]
    assert np.all(z == 0.0) and not np.signbit(z).any()
    assert not got["wx"][:, -1].any() and not got["gx"][:, -1].any() and not got["wy"][-1].any() and not got["gy"][-1].any()


def test_no_fixed_pixels():
    p, _, G = problem(12)
    for fixed in (np.zeros((H, W), bool), None):
        got = compare(p, fixed, G)
        assert not got["values"].any()


def test_every_pixel_fixed():
    p, _, G = problem(13)
    fixed = np.ones((H, W), bool)
    u, v, got = ah.dense_reference(G, fixed=fixed, **p)
    assert np.array_equal(u, p["values"]) and not v.any()
    assert np.array_equal(got["values"], G)                      # u = values: dL/dvalues = G, every other gradient 0
    for name in ("wx", "wy", "lam", "gx", "gy", "f"):
        assert not got[name].any(), name
    compare(p, fixed, G)


def test_dead_pixels():
    """A pixel with lambda = 0 and four zero weights has an empty row: it keeps u = 0 and v = 0, and L jumps when one of
    its weights becomes non-zero, so the weights that touch it (and its lambda) have no derivative: they are left out of
    the differences.  Everything else still matches, including the edges' gx, gy whose gradient w * s is 0 there."""
    p, fixed, G = problem(14)
    dead = np.zeros((H, W), bool)
    dead[2, 2:4] = True
    fixed &= ~dead
    p["lam"][dead] = 0.0
    p["wx"][2, 1:4] = 0.0
    p["wy"][1:3, 2:4] = 0.0
    lv = ch.level0(W, H, p["wx"], p["wy"], p["lam"], fixed)
    assert np.array_equal(~lv.live & ~fixed, dead)
    touch_x = np.zeros((H, W), bool)
    touch_x[2, 1:4] = True
    touch_y = np.zeros((H, W), bool)
    touch_y[1:3, 2:4] = True
    u, v, _ = ah.dense_reference(G, fixed=fixed, **p)
    assert not u[dead].any() and not v[dead].any()
    compare(p, fixed, G, skip={"wx": touch_x, "wy": touch_y, "lam": dead})
    b, x = ah.begin(lv.live, fixed, G)
    assert not b[dead].any() and not b[fixed].any() and np.array_equal(b[lv.live], G[lv.live]) and not x.any()


def test_model_reads_x_as_zero_at_fixed_pixels():
    p, fixed, G = problem(15)
    r = np.random.default_rng(16)
    x, u = r.uniform(-1, 1, (H, W, C)), r.uniform(-1, 1, (H, W, C))
    a = ah.gradients(x, u, G, fixed=fixed, **{k: p[k] for k in ("gx", "gy", "f", "wx", "wy", "lam")})
    x2 = np.where(fixed[..., None], 77.0, x)
    b = ah.gradients(x2, u, G, fixed=fixed, **{k: p[k] for k in ("gx", "gy", "f", "wx", "wy", "lam")})
    for name in a:
        assert np.array_equal(a[name], b[name]), name
