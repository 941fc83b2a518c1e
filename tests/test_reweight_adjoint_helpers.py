"""CPU: the numpy model of the reweight adjoint (tests/reweight_adjoint_helpers.py) against itself and against central
differences: `vjp` has `vjp_scalar`'s bits; it is the derivative of reweight_helpers.weights / robust_helpers.data_weights;
and chained with adjoint_helpers.dense_reference it is the gradient of a dense IRLS loop.

Input condition of the difference tests: every argument of phi keeps |sqrt(q) - eps| >= 1e-3 and q > 0 (the Huber kink and
the reciprocal's q = 0 are where the penalties are not differentiable); reweight_adjoint_helpers.margins asserts it on the
reference alone, and the committed seeds are chosen so that it holds.

Tolerances.  Central differences at h = 1e-6, compared as max |numeric - analytic| / max |analytic| per gradient.  Measured
over the committed seeds: 1.70e-9 for `vjp` (allowed: 1.70e-8) and 1.14e-8 for the chained gradient (allowed: 1.14e-7); NOTES R41.1
has both."""
import itertools

import numpy as np
import pytest

import reweight_adjoint_helpers as rah
import reweight_helpers as rh
import robust_helpers as bh

EPS, DEPS, SCALE, DSCALE, STEP = 0.05, 0.08, 0.75, 1.25, 1e-6
VJP_TOL, CHAIN_TOL = 1.70e-8, 1.14e-7                        # 10 x the measured 1.70e-9 and 1.14e-8
EDGE_CASES = rh.PAIRS + [("quadratic", "edge"), ("quadratic", "pixel")]
DATA = (None,) + bh.PENALTIES
# (H, W, C, per channel) -> the seed whose inputs meet the input condition
SEEDS = {(5, 7, 2, False): 1, (5, 7, 2, True): 3, (1, 6, 1, False): 1, (1, 6, 1, True): 1, (6, 1, 3, False): 1, (6, 1, 3, True): 1}


def make(H, W, C, per_channel):
    r = np.random.default_rng(SEEDS[(H, W, C, per_channel)])
    shape = (H, W, C) if per_channel else (H, W)
    a = dict(u=r.uniform(0, 1, (H, W, C)), gx=0.1 * r.standard_normal((H, W, C)), gy=0.1 * r.standard_normal((H, W, C)),
             f=r.uniform(0, 1, (H, W, C)), base_wx=r.uniform(0.5, 2, shape), base_wy=r.uniform(0.5, 2, shape), lam=r.uniform(0.5, 2, shape),
             grad_wx=r.standard_normal(shape), grad_wy=r.standard_normal(shape), grad_lambda=r.standard_normal(shape))
    gap, qmin = rah.margins(a["u"], a["gx"], a["gy"], EPS, dict(f=a["f"], penalty="huber", eps=DEPS), per_channel)
    assert gap >= 1e-3 and qmin > 0.0, (gap, qmin)
    return a


def both(a, penalty, coupling, data_penalty, per_channel, fn):
    data = None if data_penalty is None else dict(f=a["f"], penalty=data_penalty, scale=DSCALE, eps=DEPS, base=a["lam"])
    return fn(a["u"], a["gx"], a["gy"], penalty, coupling, SCALE, EPS, a["base_wx"], a["base_wy"], per_channel, a["grad_wx"], a["grad_wy"],
              data, a["grad_lambda"] if data is not None else None)


def test_array_and_scalar_models_give_the_same_bits():
    n = 0
    for (H, W, C, per_channel), (penalty, coupling) in itertools.product(SEEDS, EDGE_CASES):
        for data_penalty in DATA:
            if penalty == "quadratic" and data_penalty is None:
                continue
            a = make(H, W, C, per_channel)
            va, vs = both(a, penalty, coupling, data_penalty, per_channel, rah.vjp), both(a, penalty, coupling, data_penalty, per_channel, rah.vjp_scalar)
            for name in rah.OUTPUTS:
                if va[name] is None:
                    assert vs[name] is None and data_penalty is None
                    continue
                assert np.array_equal(va[name].view(np.uint64), vs[name].view(np.uint64)), (H, W, C, per_channel, penalty, coupling, data_penalty, name)
            n += 1
    assert n == 6 * (6 * 5 + 2 * 4)


def loss(a, penalty, coupling, data_penalty, per_channel):
    wx, wy = bh.edge_weights(a["u"], a["gx"], a["gy"], penalty, coupling, SCALE, EPS, a["base_wx"], a["base_wy"], per_channel)
    total = (a["grad_wx"] * wx).sum() + (a["grad_wy"] * wy).sum()
    if data_penalty is not None:
        total += (a["grad_lambda"] * bh.data_weights(a["u"], a["f"], data_penalty, DSCALE, DEPS, a["lam"], per_channel)).sum()
    return total


def central(fn, x):
    """d fn / d x by central differences, entry by entry"""
    num = np.zeros_like(x)
    for idx in np.ndindex(x.shape):
        p, m = x.copy(), x.copy()
        p[idx] += STEP
        m[idx] -= STEP
        num[idx] = (fn(p) - fn(m)) / (2.0 * STEP)
    return num


def gap(numeric, analytic):
    return float(np.abs(numeric - analytic).max() / np.abs(analytic).max()) if np.abs(analytic).max() > 0.0 else float(np.abs(numeric).max())


@pytest.mark.parametrize("key", list(SEEDS), ids=lambda k: f"{k[0]}x{k[1]}x{k[2]}{'pc' if k[3] else ''}")
def test_vjp_is_the_derivative_of_the_weights(key):
    H, W, C, per_channel = key
    a = make(H, W, C, per_channel)
    worst = 0.0
    for penalty, coupling in EDGE_CASES:
        for data_penalty in DATA:
            if penalty == "quadratic" and data_penalty is None:
                continue
            v = both(a, penalty, coupling, data_penalty, per_channel, rah.vjp)
            names = {"g_u": "u", "g_gx": "gx", "g_gy": "gy", "g_base_wx": "base_wx", "g_base_wy": "base_wy"}
            if data_penalty is not None:
                names.update(g_f="f", g_lambda="lam")
            for out, name in names.items():
                num = central(lambda x: loss(dict(a, **{name: x}), penalty, coupling, data_penalty, per_channel), a[name])
                d = gap(num, v[out])
                worst = max(worst, d)
                assert d <= VJP_TOL, (key, penalty, coupling, data_penalty, out, d)
    print(f"vjp against central differences {key}: worst {worst:.3g}")


# ---- the chained gradient of a dense IRLS loop ---------------------------------------------------------------------------
K, CW, CH, CC = 3, 8, 6, 2


def chain_inputs(seed):
    r = np.random.default_rng(seed)
    f = rh.step_image(CW, CH, CC, seed, noise=0.1)
    return dict(f=f, gx=0.1 * r.standard_normal((CH, CW, CC)), gy=0.1 * r.standard_normal((CH, CW, CC)), G=r.standard_normal((CH, CW, CC)),
                lam=r.uniform(0.5, 1.5, (CH, CW)), base_wx=r.uniform(0.5, 2.0, (CH, CW)), values=r.uniform(0, 1, (CH, CW, CC)),
                fixed=(r.random((CH, CW)) < 0.15).astype(np.uint8))


def run_chain(name, seed, penalty, coupling, strength, eps, wrt, forward, **kw):
    """analytic against central differences of `forward(**inputs) -> u_K` for every input named in wrt"""
    a = chain_inputs(seed)
    if kw.pop("scalar_data_weight", False):                     # (dense_irls takes a number: its gradient is the plane's sum)
        a["lam"] = np.array(0.8)
    args = dict(data_weight=a["lam"], **{n: a[n] for n in kw.pop("use", ())}, **kw)
    _, steps = rah.dense_unrolled(a["f"], a["gx"], a["gy"], penalty, coupling, strength, eps, K, **args)
    # the condition at every step's reweight (step 0 of a robust loop reweights from u = f with a quadratic data term)
    for k, (u_in, _, _, _, data) in enumerate(steps):
        d = None if data is None or data["penalty"] == "quadratic" else dict(f=a["f"], penalty=data["penalty"], eps=kw.get("data_eps"))
        g, q = rah.margins(u_in, a["gx"], a["gy"], eps, d, False)
        assert g >= 1e-3 and q > 0.0, (name, k, g, q)
    _, grads = rah.dense_unrolled_gradients(a["G"], a["f"], a["gx"], a["gy"], penalty, coupling, strength, eps, K, **args)
    worst = 0.0
    for n in wrt:
        x = a["lam"] if n == "data_weight" else a[n]
        num = central(lambda v: float((a["G"] * forward(dict(a, **{("lam" if n == "data_weight" else n): v}))).sum()), x)
        d = gap(num, grads[n] if x.ndim else grads[n].sum())
        worst = max(worst, d)
        assert d <= CHAIN_TOL, (name, n, d)
    print(f"chained gradient against central differences, {name}: worst {worst:.3g}")


def test_chain_tv_against_dense_irls():
    fwd = lambda a: rh.dense_irls(a["f"], a["gx"], a["gy"], "charbonnier", "pixel", 0.3, EPS, a["lam"], K)[0][-1]
    run_chain("tv", 11, "charbonnier", "pixel", 0.3, EPS, ("f", "gx", "gy", "data_weight"), fwd, scalar_data_weight=True)


def test_chain_huber_edge_with_a_fixed_mask_and_base_weights():
    fwd = lambda a: rah.dense_unrolled(a["f"], a["gx"], a["gy"], "huber", "edge", 0.3, EPS, K, data_weight=a["lam"], base_wx=a["base_wx"],
                                       values=a["values"], fixed=a["fixed"])[0][-1]
    run_chain("huber / edge, fixed", 3, "huber", "edge", 0.3, EPS, ("f", "gx", "gy", "data_weight", "values", "base_wx"), fwd,
              use=("base_wx", "values", "fixed"))


def test_chain_tv_l1_against_dense_irls_robust():
    def fwd(a):
        # dense_irls_robust takes the data weight as a number: the plane enters through data_scale = 1 and ... a uniform plane
        return rah.dense_unrolled(a["f"], a["gx"], a["gy"], "charbonnier", "pixel", 0.3, EPS, K, data_weight=a["lam"], data_penalty="charbonnier",
                                  data_eps=DEPS)[0][-1]
    run_chain("tv-l1", 20, "charbonnier", "pixel", 0.3, EPS, ("f", "gx", "gy", "data_weight"), fwd, data_penalty="charbonnier", data_eps=DEPS)
    # the loop differentiated above is dense_irls_robust's: the same iterates for a uniform data weight
    a = chain_inputs(20)
    mine = rah.dense_unrolled(a["f"], a["gx"], a["gy"], "charbonnier", "pixel", 0.3, EPS, K, data_weight=0.8, data_penalty="charbonnier",
                              data_eps=DEPS)[0]
    theirs = bh.dense_irls_robust(a["f"], a["gx"], a["gy"], "charbonnier", "pixel", 0.3, EPS, "charbonnier", 0.8, DEPS, K)[0]
    for m, t in zip(mine, theirs):
        assert np.allclose(m, t, rtol=1e-12, atol=1e-13)
