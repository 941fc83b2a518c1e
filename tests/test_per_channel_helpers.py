"""CPU: the systems of the per-channel-operator tests (tests/per_channel_helpers.py) are what the GPU tests rely on: on
the rescaled hierarchy, nu = 2, to 1e-10 ||b||, cap 200, every channel converges, and at least three channels of a
handle stop at different iterations -- which is what exercises the per-channel `active` flags of the batched loop.

The counts below are the numpy model's (constrained_helpers.pcg) on these helpers' systems."""
import numpy as np
import pytest

import per_channel_helpers as pch

COUNTS = {(131, 67, 3): [6, 79, 13], (70, 37, 5): [6, 55, 13, 45, 9], (40, 24, 2): [6, 44], (5, 3, 2): [4, 5]}


@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_every_channel_converges_at_its_own_iteration(W, H, C):
    got = pch.solve_counts(W, H, C)
    print(f"{W}x{H}x{C}: {got}")
    assert all(conv for _, conv in got), got
    assert [its for its, _ in got] == COUNTS[(W, H, C)]
    assert len(set(its for its, _ in got)) >= min(C, 3)                 # three channels (two where C = 2) stop apart


@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_the_counts_of_one_call_on_a_handle(W, H, C):
    """The same systems as a handle solves them: one epsilon, 1e-10 ||b_0||, from the assembled start vector.  These are
    the counts the GPU tests hold the sequential and the batched solve to."""
    got = pch.solve_counts(W, H, C, as_handle=True)
    assert all(conv for _, conv in got), got
    assert [its for its, _ in got] == pch.HANDLE_COUNTS[(W, H, C)]
    assert len(set(pch.HANDLE_COUNTS[(W, H, C)])) >= min(C, 3)


def test_the_channels_are_what_the_module_says():
    W, H, C = 70, 37, 5
    wx, wy, lam, fixed = pch.operators(W, H, C)
    assert wx.dtype == wy.dtype == lam.dtype == np.float32 and fixed.dtype == np.uint8
    assert np.all(wx[..., 0] == 1) and np.all(lam[..., 0] == np.float32(1e-2))
    assert np.array_equal(wx[..., 1], wx[..., 3]) and np.all(lam[..., 1] == 1)
    assert 0.1 <= wx[..., 2].min() and wx[..., 2].max() <= 10 and 0 < (lam[..., 2] == 10).mean() < 0.03
    assert not fixed[..., :3].any() and fixed[..., 3].any() and fixed[..., 4].any()
    assert not np.array_equal(fixed[..., 3], fixed[..., 4])
    # channel 4 has dead free pixels (the block) and anchors inside and outside it
    lv = pch.channel_levels((wx, wy, lam, fixed), 4)[0]
    dead = (lv.d == 0) & ~lv.fixed
    assert dead.sum() > 50 and (lv.fixed & (lam[..., 4] == 0)).any() and (lv.fixed & (lam[..., 4] != 0)).any()
    # no other channel has a dead pixel
    for c in range(4):
        lv = pch.channel_levels((wx, wy, lam, fixed), c)[0]
        assert not ((lv.d == 0) & ~lv.fixed).any(), c


def test_shape_fixed_is_line_helpers_where_it_fits():
    import line_helpers as lh
    assert np.array_equal(pch.shape_fixed(131, 67), lh.shape_fixed(131, 67))
    f = pch.shape_fixed(70, 37)
    assert f.shape == (37, 70) and f[37 // 3].all() and f[:, 70 // 4].all() and f[37 // 2, 70 // 2] == 1 and not f.all()
