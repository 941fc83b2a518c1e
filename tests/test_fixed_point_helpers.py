"""CPU: the models of tests/fixed_point_helpers.py against the models the repository already trusts.

The implicit gradient is the unrolled one's limit.  On 8 x 6 x 2 (Charbonnier / pixel with base weights, a lambda plane and
three fixed pixels, plain and with a Charbonnier data term; Huber / edge) dense_fixed_point_gradients -- 200 exact forward
steps, then the z iteration with exact adjoint solves -- equals reweight_adjoint_helpers.dense_unrolled_gradients at
outer = 200, every one of the seven gradients.  Measured, max |a - b| / max |b|: 2.1e-15 (tv, d/dgy), 4.2e-15 (tv_l1, d/dgy),
2.4e-15 (huber, d/dgx); allowed: 10 x the worst, 4.2e-14.

Input condition, asked of the reference alone: the dense forward's last update <= 1e-12 and the dense z iteration's last
||z_new - z_old|| <= 1e-12 ||G||, within 200 steps on 8 x 6 and within fixed_point_helpers.STEPS on 16 x 12 x 2 (the step
counts the GPU tests use, plus a margin); the Huber case keeps every |sqrt(q) - epsilon| >= 1e-5 on its iterates."""
import numpy as np
import pytest

import fixed_point_helpers as fp
import reweight_adjoint_helpers as rah

MEASURED = 4.2e-15
ALLOWED = 10.0 * MEASURED


def wide(a):
    return a["gx"].astype(np.float64), a["gy"].astype(np.float64)


@pytest.mark.parametrize("name", list(fp.CASES))
def test_the_fixed_point_gradient_is_the_unrolled_gradients_limit(name):
    penalty, coupling = fp.CASES[name][:2]
    a = fp.case_inputs(name, 8, 6)
    gx, gy = wide(a)
    kw = fp.case_kw(name, a)
    assert int(np.count_nonzero(a["fixed"])) == 3
    u, got, info = fp.dense_fixed_point_gradients(a["G"], a["f"], gx, gy, penalty, coupling, fp.STRENGTH, fp.EPS, 200, 200, **kw)
    assert info["forward_update"] <= 1e-12 and info["history"][-1][0] <= 1e-12 * np.linalg.norm(a["G"])
    gap, qmin = rah.margins(u, gx, gy, fp.EPS)
    assert qmin > 0.0 and (penalty != "huber" or gap >= fp.KINK), (name, gap, qmin)
    u_ref, ref = rah.dense_unrolled_gradients(a["G"], a["f"], gx, gy, penalty, coupling, fp.STRENGTH, fp.EPS, 200, **kw)
    assert np.array_equal(u, u_ref)
    for n in fp.NAMES:
        gap = fp.relative_gap(got[n], ref[n])
        print(f"{name}: d/d{n} differs from the unrolled gradient by {gap:.3g}")
        assert gap <= ALLOWED, (name, n, gap)


@pytest.mark.parametrize("name", list(fp.CASES))
def test_the_step_counts_of_the_gpu_tests_reach_the_fixed_point(name):
    penalty, coupling = fp.CASES[name][:2]
    a = fp.case_inputs(name, 16, 12)
    gx, gy = wide(a)
    forward, backward = fp.STEPS[name]
    iterates, _ = rah.dense_unrolled(a["f"], gx, gy, penalty, coupling, fp.STRENGTH, fp.EPS, forward, **fp.case_kw(name, a))
    assert float(np.abs(iterates[-1] - iterates[-2]).max()) <= 1e-12
    if penalty == "huber":
        assert min(rah.margins(u, gx, gy, fp.EPS)[0] for u in iterates) >= fp.KINK
    _, history = fp.fixed_point_gradients(iterates[-1], a["G"], a["f"], gx, gy, penalty, coupling, fp.STRENGTH, fp.EPS, backward,
                                          **fp.case_kw(name, a))
    print(f"{name}: last forward update {np.abs(iterates[-1] - iterates[-2]).max():.3g}, last |dz| / |G| "
          f"{history[-1][0] / np.linalg.norm(a['G']):.3g}")
    assert history[-1][0] <= 1e-12 * np.linalg.norm(a["G"])
    rates = [history[k + 1][0] / history[k][0] for k in range(4, backward - 1)]
    assert max(rates) < 1.0                                   # linear, as the forward loop


def test_step_on_an_operator_per_channel_is_the_one_channel_step_per_channel():
    r = np.random.default_rng(5)
    H, W, C = 5, 7, 3
    u, v, z, G = (r.standard_normal((H, W, C)) for _ in range(4))
    gx, gy = (r.standard_normal((H, W, C)).astype(np.float32) for _ in range(2))
    bwx, bwy, base = (r.uniform(0.5, 2.0, (H, W, C)) for _ in range(3))
    fixed = (r.random((H, W, C)) < 0.15).astype(np.uint8)
    f = r.standard_normal((H, W, C))
    data = dict(f=f, penalty="huber", scale=0.7, eps=0.3, base=base)
    b, report, full = fp.step(v, z, u, G, "charbonnier", "pixel", 0.3, 0.05, gx, gy, bwx, bwy, True, data, fixed)
    for c in range(C):
        s = slice(c, c + 1)
        one = dict(data, f=f[:, :, s], base=base[:, :, c])
        bc, rc, fc = fp.step(v[:, :, s], z[:, :, s], u[:, :, s], G[:, :, s], "charbonnier", "pixel", 0.3, 0.05, gx[:, :, s], gy[:, :, s],
                             bwx[:, :, c], bwy[:, :, c], False, one, fixed[:, :, c])
        assert np.array_equal(b[:, :, s], bc) and np.array_equal(report[c], rc[0]) and np.array_equal(full[:, :, s], fc)
    assert np.all(b[fixed != 0] == 0.0) and np.any(full[fixed != 0] != 0.0)
