"""GPU: the rows a wide depth-8 tile reads and writes (ccp_grid_fused_wide.hpp), now that a ring turn of 20 march
steps goes through one buffer descriptor per plane (ccp_wide_plan.hpp, wide_turn_rows) instead of one per row.
Bit for bit against the 128-px strips (CCP_GS_WIDE=0) and against the CPU oracle: no tolerance.

The smallest shapes where row addressing can go wrong: one wide strip (W = 449) and two with the last one clipped
(W = 673), chunks of 16 rows, and heights that move the rows of the interior and of its halo through the residues around
a multiple of the ring's 20 rows and of 2, so that turns begin before the first loaded row and end after the last.
Calls of 8 sweeps, of 16 (two depth-8 passes: the first stores no red, the second does) and both in a row; the
planner's segments and 1, 2 and 3 forced ones (joins at both parities, a tile clipped at the top and at the bottom).
(A handle whose buffers may not swap runs an even number of passes per call, so its call of 8 sweeps is two depth-4
passes on the 128-px strips: that call checks the routes against each other and sets the state the next call's wide
passes start from.)  One pair of row blocks whose
second block starts at an odd image row: its tiles march from the row before their first loaded row.
"""
import functools

import numpy as np
import pytest

import rowblock_sweep_helpers as rsh

pytestmark = pytest.mark.gpu

T = 8
ROWS = 16
WIDTHS = [449, 673]
HEIGHTS = [97, 98, 99, 115, 116, 117, 118, 135, 136, 137]
CALLS = [[8], [16], [8, 16]]
MODES = [None, 1, 2, 3]                    # CCP_GS_WIDE_SEGMENTS: unset (the planner), forced counts
SEED = 57


@pytest.fixture(scope="module")
def capi():
    from coursecomputationalphotography_amd import capi
    assert capi.device_count() >= 1
    return capi


@functools.lru_cache(maxsize=None)
def system(W, H):
    from coursecomputationalphotography_amd import synth
    b = synth.poisson_system(W, H, SEED)[0]
    b.setflags(write=False)
    return b


_oracle = {}


def oracle_x(orc, W, H, iters):
    """the oracle's iterate after `iters` sweeps from x = 1 (computed once per shape and count, never changed)"""
    key = (W, H, iters)
    if key not in _oracle:
        import oracle
        from coursecomputationalphotography_amd import synth
        v, c, r = synth.poisson_csr(W, H)
        x = orc.multicolour_gauss_seidel(v, c, r, oracle.grid_colour(W, H), system(W, H), 0.0, iters)[0]
        x.setflags(write=False)
        _oracle[key] = x
    return _oracle[key]


def run(capi, monkeypatch, W, H, calls, mode, wide=True, trace=None):
    monkeypatch.setenv("CCP_GS_WIDE", "1" if wide else "0")
    monkeypatch.setenv("CCP_GS_MULTI", "0")
    monkeypatch.delenv("CCP_GS_RED_STORE", raising=False)
    if mode is None:
        monkeypatch.delenv("CCP_GS_WIDE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("CCP_GS_WIDE_SEGMENTS", str(mode))
    if trace:
        monkeypatch.setenv("CCP_GS_TRACE_FILE", trace)
    else:
        monkeypatch.delenv("CCP_GS_TRACE_FILE", raising=False)
    g = capi.Grid(W, H, 1)
    g.set_b(system(W, H), 0)
    g.fill_x(1.0)
    g.set_tiling(T, ROWS)
    out = []
    for n in calls:
        g.sweep(n)
        out.append(g.get_x(0).ravel().copy())
    g.synchronize()
    g.close()
    return out


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_rows_equal_narrow_and_oracle(capi, orc, monkeypatch, tmp_path, W, H):
    for calls in CALLS:
        narrow = run(capi, monkeypatch, W, H, calls, None, wide=False)
        done = 0
        for k, n in enumerate(calls):
            done += n
            assert np.array_equal(narrow[k], oracle_x(orc, W, H, done)), (W, H, calls, k)
        for mode in MODES:
            trace = str(tmp_path / f"trace_{len(calls)}_{calls[0]}_{mode}.bin")
            got = run(capi, monkeypatch, W, H, calls, mode, trace=trace)
            passes = rsh.wide_passes(trace)
            # every depth-8 pass ran the wide kernel: two per 16 sweeps of a call
            assert len(passes) == sum(2 * (n // (2 * T)) for n in calls), (W, H, calls, mode, len(passes))
            if mode is not None:
                assert all(max(t[0] for t in tiles) + 1 <= mode for tiles in passes), (W, H, mode)
            for k, (a, b) in enumerate(zip(got, narrow)):
                bad = np.flatnonzero(a != b)
                if bad.size:
                    print(f"W {W} H {H} calls {calls} segments {mode} call {k}: {bad.size} values differ, rows "
                          f"{sorted(set((bad // W).tolist()))[:40]}")
                assert np.array_equal(a, b), (W, H, calls, mode, k)


def test_row_block_with_an_odd_first_row(capi, orc, monkeypatch, tmp_path):
    """The second block's local row 0 is image row 49: a tile whose first loaded row m0 is even starts its march at
    m0 - 1, a row that does not exist."""
    W, H, cuts, ghost, sweeps = 449, 180, [0, 81, 180], 32, [16, 16]
    assert rsh.first_local_rows(cuts, ghost) == [0, 49]
    bs = [system(W, H)]
    for mode in MODES:
        for v in ("CCP_GS_WIDE", "CCP_GS_RED_STORE", "CCP_GS_WIDE_SEGMENTS", "CCP_GS_TRACE_FILE"):
            monkeypatch.delenv(v, raising=False)
        monkeypatch.setenv("CCP_GS_MULTI", "0")
        if mode is not None:
            monkeypatch.setenv("CCP_GS_WIDE_SEGMENTS", str(mode))
        paths = []

        def make(W, H, C, row_begin, row_count, ghost):
            paths.append(str(tmp_path / f"trace_{mode}_{row_begin}.bin"))
            monkeypatch.setenv("CCP_GS_TRACE_FILE", paths[-1])
            return capi.Grid(W, H, C, row_begin, row_count, ghost)

        got = rsh.run_intervals(W, H, 1, cuts, ghost, sweeps, bs, tiling=(T, ROWS), factory=make)
        assert len(rsh.wide_passes(paths[1])) >= 1, "the wide kernel did not run on the block with the odd first row"
        done = 0
        for k, n in enumerate(sweeps):
            done += n
            assert np.array_equal(np.asarray(got[k][0]).ravel(), oracle_x(orc, W, H, done)), (mode, k)
