"""CPU: the manual-exchange driver behind test_gpu_rowblock_depth8.py is sound (rowblock_sweep_helpers.py).  Driven with a
numpy stand-in for the handle, the blocked run gives the bits of the stand-in on the whole image after every refresh
interval, for the very cuts, ghosts and sweep counts of the GPU cases; a stale ghost row that reached an owned row, a row
written back to the wrong place or a missed refresh would show.  The driver refuses a count the ghosts cannot carry,
and every case said to have a block on an odd first local row has one."""
import numpy as np
import pytest

import rowblock_sweep_helpers as rsh


def rhs(W, H, C, seed):
    rng = np.random.Generator(np.random.MT19937(seed))
    return [rng.uniform(-1.0, 1.0, W * H) * 10.0 ** (ch - 1) for ch in range(C)]


@pytest.mark.parametrize("name", sorted(rsh.CASES))
def test_blocks_equal_the_whole_image(name):
    W, H, C, cuts, ghost, _, sweeps, _ = rsh.CASES[name]
    bs = rhs(W, H, C, 5)
    got = rsh.run_intervals(W, H, C, cuts, ghost, sweeps, bs, factory=rsh.NumpyBlock)
    whole = rsh.NumpyBlock(W, H, C, 0, H, 0)
    for ch in range(C):
        whole.set_b(bs[ch], ch)
    whole.fill_x(1.0)
    assert len(got) == len(sweeps)
    for k, n in enumerate(sweeps):
        whole.sweep(n)
        for ch in range(C):
            assert got[k][ch].shape == (H, W)
            assert np.array_equal(got[k][ch], whole.x[ch]), (name, k, ch)


def test_a_stale_row_would_show():
    """The stand-in does go wrong next to a stale edge: without the refresh the same counts give other bits."""
    W, H, C, cuts, ghost = 37, 60, 1, [0, 21, 40, 60], 8
    bs = rhs(W, H, C, 9)
    whole = rsh.NumpyBlock(W, H, C, 0, H, 0)
    whole.set_b(bs[0])
    whole.fill_x(1.0)
    whole.sweep(8)
    assert np.array_equal(rsh.run_intervals(W, H, C, cuts, ghost, [4, 4], bs, factory=rsh.NumpyBlock)[1][0], whole.x[0])

    class NoRefresh(rsh.NumpyBlock):
        def set_x(self, rows, channel=0):
            pass

    assert not np.array_equal(rsh.run_intervals(W, H, C, cuts, ghost, [4, 4], bs, factory=NoRefresh)[1][0], whole.x[0])


def test_refuses_more_sweeps_than_the_ghosts_carry():
    W, H, C, cuts, ghost = 19, 30, 1, [0, 11, 30], 6
    bs = rhs(W, H, C, 2)
    rsh.run_intervals(W, H, C, cuts, ghost, [3], bs, factory=rsh.NumpyBlock)
    with pytest.raises(ValueError):
        rsh.run_intervals(W, H, C, cuts, ghost, [3, 4], bs, factory=rsh.NumpyBlock)
    with pytest.raises(ValueError):
        rsh.RowBlocks(W, H, C, [0, 11, 29], ghost, bs, factory=rsh.NumpyBlock)


@pytest.mark.parametrize("name", sorted(rsh.CASES))
def test_odd_cases_have_an_odd_first_local_row(name):
    W, H, C, cuts, ghost, rows, sweeps, odd = rsh.CASES[name]
    first = [cuts[i] - min(ghost, cuts[i]) for i in range(len(cuts) - 1)]
    assert first == rsh.first_local_rows(cuts, ghost)
    assert any(f & 1 for f in first) == odd, first
    assert name == "F" or odd                              # A to E are the odd cases of the issue
    assert all(2 * n <= ghost for n in sweeps) and rows % 2 == 0
    # the stand-in's geometry is the handle's: first_local_row, local_rows
    for i, f in enumerate(first):
        g = rsh.NumpyBlock(W, H, C, cuts[i], cuts[i + 1] - cuts[i], ghost)
        assert g.first_local_row == f
        assert g.local_rows == min(cuts[i + 1] + ghost, H) - f


def test_trace_reader(tmp_path):
    """trace_passes / wide_passes on a hand-made file: two passes, idle slots dropped, fields unpacked."""
    def rec(kernel, seg, strip, ch, end=7):
        return [5, end, 0, seg | (strip << 16) | (ch << 32) | (kernel << 40)]
    p1 = rec(3, 0, 0, 0) + rec(3, 1, 2, 1) + rec(3, 9, 9, 9, end=0) + rec(1, 4, 5, 0)
    p2 = rec(0, 2, 3, 0)
    raw = []
    for depth, p in ((8, p1), (4, p2)):
        raw += [rsh.TRACE_MAGIC, depth, 1, 1, 1, 1, len(p), 32] + p
    path = tmp_path / "t.bin"
    np.array(raw, dtype=np.uint64).tofile(path)
    assert rsh.trace_passes(path) == [(8, [(3, 0, 0, 0), (3, 1, 2, 1), (1, 4, 5, 0)]), (4, [(0, 2, 3, 0)])]
    assert rsh.wide_passes(path) == [[(0, 0, 0), (1, 2, 1)]]
    assert [rsh.wide_strips(W) for W in (449, 673, 898, 1001)] == [2, 3, 4, 4]


def test_depth8_passes_of_the_cases():
    """The restated tiling (depth8_passes): every depth-8 pass of every block of A to E has ordinary chunks and so a wide
    interior, and the situations the cases were chosen for are there."""
    passes = {}
    for name in "ABCDE":
        W, H, C, cuts, ghost, rows, sweeps, _ = rsh.CASES[name]
        assert all(n % 8 == 0 for n in sweeps)             # (an even number of depth-8 passes is the only cheapest plan)
        passes[name] = rsh.depth8_passes(H, cuts, ghost, rows, sweeps[0] // 8)
        assert rsh.wide_strips(W) >= 1
        for block in passes[name]:
            for st_lo, st_hi, interior in block:
                assert interior is not None and interior[3] - interior[2] >= 2, (name, st_lo, st_hi)
                assert interior[2] % 2 == 0 and st_lo % 2 == 0
    # A, the middle block: no border chunk row at all, the interior is the stored range and starts at 16, 32, 48, 64
    assert [(lo, hi, i) for lo, hi, i in passes["A"][1]] == [(s, 263 - s, (0, 0, s, 263 - s)) for s in (16, 32, 48, 64)]
    # ... the top and the bottom block: one image edge (border chunk rows there), one stale edge
    assert all(i[0] >= 1 and i[1] == 0 and hi == 197 - 16 * (k + 1) for k, (lo, hi, i) in enumerate(passes["A"][0]))
    assert all(i[0] == 0 and i[1] >= 1 and lo == 16 * (k + 1) for k, (lo, hi, i) in enumerate(passes["A"][2]))
    # E, the 20-row block: the stored range ends as its owned rows alone, less than the 2 x 16 halo rows a tile marches
    lo, hi, _ = passes["E"][1][-1]
    assert (lo, hi) == (64, 84) and hi - lo == 20 < 32
    # D: a cut-short chunk row (32 rows) at the image's bottom, chunks of 48 elsewhere
    assert passes["D"][3][0][2] == (0, 1, 16, 250) and passes["D"][3][0][1] == 282
