"""CPU: the numpy model of ccp_grid_reweight_robust_device (tests/robust_helpers.py) against the header's text as a scalar
loop, and the IRLS loop it stands for on the outlier image with exact inner solves: the energy does not rise from the
second step on, and the robust data term at least halves the error the quadratic one leaves."""
import numpy as np
import pytest

import reweight_helpers as rh
import robust_helpers as bh


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("penalty", bh.PENALTIES)
def test_vector_and_scalar_models_agree_bit_for_bit(penalty, per_channel):
    rng = np.random.default_rng(3)
    H, W, C = 6, 7, 3
    u = 255.0 * rng.random((H, W, C))
    f = rng.integers(0, 256, (H, W, C)).astype(np.uint8)
    f[2, 3] = 9
    u[2, 3] = 9.0                                              # a residual of exactly 0
    base = (0.5 + rng.random((H, W, C) if per_channel else (H, W))).astype(np.float32)
    for b in (None, base):
        got = bh.data_weights(u, f, penalty, 0.75, 5e-2, b, per_channel)
        want = bh.data_weights_scalar(u, f, penalty, 0.75, 5e-2, b, per_channel)
        assert got.shape == ((H, W, C) if per_channel else (H, W))
        assert np.array_equal(bits(got), bits(want)), (penalty, per_channel, b is None)
    if penalty != "quadratic":
        assert bits(bh.data_weights(u, f, penalty, 0.75, 5e-2, None, per_channel)[2, 3]).tolist() == \
               bits(np.float64(0.75) * rh.phi(np.float64(0.0), penalty, 5e-2)).tolist() * (C if per_channel else 1)


def test_quadratic_is_the_scale_and_leaves_a_base_alone():
    u = np.random.default_rng(1).random((4, 5, 2))
    base = np.random.default_rng(2).random((4, 5))
    assert np.array_equal(bits(bh.data_weights(u, None, "quadratic", 1.0, None, base)), bits(base))
    assert (bh.data_weights(u, None, "quadratic", 0.25, None) == 0.25).all()
    wx, wy = bh.edge_weights(u, None, None, "quadratic", "pixel", 0.5, 1e-2)
    assert (wx[:, :-1] == 0.5).all() and (wy[:-1] == 0.5).all() and not bits(wx[:, -1]).any() and not bits(wy[-1]).any()


@pytest.fixture(scope="module")
def runs():
    """(robust, quadratic) dense IRLS on the 16 x 12 x 2 outlier image, per case"""
    clean, noisy = bh.outlier_image(16, 12)
    out = {}
    for coupling, dp, per_channel in bh.CASES:
        its, en, _ = bh.dense_irls_robust(noisy, None, None, "charbonnier", coupling, bh.STRENGTH, bh.EPS, dp, bh.DATA_SCALE, bh.DATA_EPS,
                                          bh.OUTER, per_channel)
        quad, _ = rh.dense_irls(noisy, None, None, "charbonnier", coupling, bh.STRENGTH, bh.EPS, bh.DATA_SCALE, bh.OUTER, per_channel)
        out[(coupling, dp, per_channel)] = (clean, noisy, its, en, quad)
    return out


@pytest.mark.parametrize("case", bh.CASES)
def test_the_energy_does_not_rise_from_the_second_step_on(runs, case):
    _, _, _, en, _ = runs[case]
    steps = np.diff(en[2:])                                    # en[k + 1] is iterate k's: from iterate 1 on
    print(case, "E", en, "largest step-to-step change", steps.max())
    assert len(steps) == bh.OUTER - 2 and (steps <= 0.0).all(), (case, en)


@pytest.mark.parametrize("case", bh.CASES)
def test_the_robust_data_term_halves_the_error(runs, case):
    clean, noisy, its, _, quad = runs[case]
    robust, quadratic = bh.rmse(its[-1], clean), bh.rmse(quad[-1], clean)
    print(case, "input", bh.rmse(noisy, clean), "robust", robust, "quadratic", quadratic, "ratio", robust / quadratic)
    assert robust <= 0.5 * quadratic, (case, robust, quadratic)


def test_a_robust_first_step_starts_from_scale_over_epsilon():
    """first_step="robust": at u = f every data residual is 0, so step 0 solves with lambda = data_scale / data_epsilon
    everywhere; first_step="quadratic" gives it lambda = data_scale"""
    _, noisy = bh.outlier_image(16, 12)
    args = (noisy, None, None, "charbonnier", "pixel", bh.STRENGTH, bh.EPS, "charbonnier", bh.DATA_SCALE, bh.DATA_EPS, 2)
    assert (bh.dense_irls_robust(*args, first_step="robust")[2][0] == bh.DATA_SCALE / bh.DATA_EPS).all()
    assert (bh.dense_irls_robust(*args, first_step="quadratic")[2][0] == bh.DATA_SCALE).all()
