"""GPU: depth-8 red-black passes on ROW BLOCKS with ghost rows against the CPU oracle (k_fused_sweep_wide, k_fused_sweep,
k_fused_border, k_fused_multi; launch_fused's shrinking stored range).  The whole-image tests never take the row-parity
branch of fused_wave_wide (base = m0 - ((y0 + m0) & 1): y0 = 0 and m0 even there); a block whose first local row is odd
does, and its first pass after a refresh marches from local row -1.  The blocks are swept on their own between halo
refreshes done by hand (rowblock_sweep_helpers.RowBlocks) and every owned row of every block must equal the oracle's
whole-image iterate after every refresh interval, bit for bit, through every route: the planner's segments, forced segment
counts, the interior chunks, the 128-px strips, both store forms, several passes per launch.  On the wide routes the
per-wave trace of every block must show the wide kernel in every depth-8 pass, every (segment, strip, channel) tile
exactly once.

The cases are rowblock_sweep_helpers.CASES (tests/test_rowblock_sweep_helpers.py checks their geometry on the CPU)."""
import functools

import numpy as np
import pytest

import rowblock_sweep_helpers as rsh

pytestmark = pytest.mark.gpu

# route: (environment, wide kernel expected and traced, CCP_GS_WIDE_SEGMENTS mode)
ROUTES = {
    "planner": ({"CCP_GS_MULTI": "0"}, True, None),
    "segments0": ({"CCP_GS_MULTI": "0", "CCP_GS_WIDE_SEGMENTS": "0"}, True, 0),
    "segments1": ({"CCP_GS_MULTI": "0", "CCP_GS_WIDE_SEGMENTS": "1"}, True, 1),
    "segments3": ({"CCP_GS_MULTI": "0", "CCP_GS_WIDE_SEGMENTS": "3"}, True, 3),
    "narrow": ({"CCP_GS_MULTI": "0", "CCP_GS_WIDE": "0"}, False, None),
    "red_store0": ({"CCP_GS_MULTI": "0", "CCP_GS_RED_STORE": "0"}, True, None),
    "red_store1": ({"CCP_GS_MULTI": "0", "CCP_GS_RED_STORE": "1"}, True, None),
    "multi": ({"CCP_GS_MULTI": "1"}, False, None),
}
SWITCHES = ["CCP_GS_MULTI", "CCP_GS_WIDE", "CCP_GS_WIDE_SEGMENTS", "CCP_GS_RED_STORE", "CCP_GS_TRACE_FILE", "CCP_GS_TMAX",
            "CCP_GS_CHUNK", "CCP_GS_FUSE", "CCP_GS_ALL_BORDER", "CCP_GS_FORCE_BORDER", "CCP_GS_SHORT_EDGES"]
SEED = 83


@pytest.fixture(scope="module")
def capi():
    from coursecomputationalphotography_amd import capi
    assert capi.device_count() >= 1
    return capi


@functools.lru_cache(maxsize=None)
def systems_of(W, H, C):
    from coursecomputationalphotography_amd import synth
    return [synth.poisson_system(W, H, SEED + ch)[0] * 10.0 ** (ch - 1) for ch in range(C)]


def systems(name):
    return systems_of(*rsh.CASES[name][:3])


_oracle = {}


def oracle_x(orc, name, total_sweeps):
    """per channel, the oracle's whole-image iterate after total_sweeps (computed once per case and count, never changed)"""
    W, H, C = rsh.CASES[name][:3]
    key = (W, H, C, total_sweeps)                  # (A and E are one system)
    if key not in _oracle:
        import oracle
        from coursecomputationalphotography_amd import synth
        got = [orc.multicolour_gauss_seidel(*synth.poisson_csr(W, H), oracle.grid_colour(W, H), b, 0.0, total_sweeps)[0]
               for b in systems(name)]
        for g in got:
            g.setflags(write=False)
        _oracle[key] = got
    return _oracle[key]


def set_route(monkeypatch, route):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in ROUTES[route][0].items():
        monkeypatch.setenv(k, v)


def traced_factory(capi, monkeypatch, tmp_path, paths):
    """every block with a CCP_GS_TRACE_FILE of its own (the handle reads the variable when it is created)"""
    def make(W, H, C, row_begin, row_count, ghost):
        paths.append(str(tmp_path / f"trace_{row_begin}.bin"))
        monkeypatch.setenv("CCP_GS_TRACE_FILE", paths[-1])
        return capi.Grid(W, H, C, row_begin, row_count, ghost)
    return make


def by_count(rows, n):
    h = -(-rows // max(n, 1))
    h += h & 1
    return -(-rows // h)


def check_trace(name, route, paths):
    """every depth-8 pass of every block ran wide: all its (segment, strip, channel) tiles, each exactly once"""
    W, H, C, cuts, ghost, rows, sweeps, _ = rsh.CASES[name]
    mode = ROUTES[route][2]
    n_wide = rsh.wide_strips(W)
    geometry = rsh.depth8_passes(H, cuts, ghost, rows, max(sweeps) // 8) if name != "F" else None
    for blk, path in enumerate(paths):
        passes = rsh.trace_passes(path)
        deep = [waves for depth, waves in passes if depth == 8]
        if name != "F":
            assert len(deep) == sum(n // 8 for n in sweeps), (name, blk, len(deep))
        else:
            assert len(deep) >= 4, (name, blk, len(deep))             # the 32-sweep interval at the least
        since_refresh = 0
        interval = iter(sweeps)
        left = next(interval) // 8
        for waves in deep:
            tiles = [w[1:] for w in waves if w[0] == rsh.KERNEL_WIDE]
            assert tiles, f"case {name}, block {blk}: a depth-8 pass without the wide kernel"
            assert all(w[0] in (rsh.KERNEL_WIDE, 1, 2) for w in waves), (name, blk)     # wide tiles and border tiles only
            n_seg = max(t[0] for t in tiles) + 1
            if geometry:
                while left == 0:
                    left, since_refresh = next(interval) // 8, 0
                _, _, (_, _, y0, y1) = geometry[blk][since_refresh]
                since_refresh, left = since_refresh + 1, left - 1
                if mode == 0:
                    assert n_seg == -(-(y1 - y0) // rows), (name, blk, n_seg, y0, y1)
                elif mode is not None:
                    assert n_seg == by_count(y1 - y0, mode), (name, blk, n_seg, y0, y1)
                else:
                    assert n_seg == by_count(y1 - y0, n_seg), (name, blk, n_seg, y0, y1)      # no empty segment
            assert len(tiles) == len(set(tiles)) == n_seg * n_wide * C, (name, blk, len(tiles), n_seg, n_wide, C)
            assert set(tiles) == {(s, w, c) for s in range(n_seg) for w in range(n_wide) for c in range(C)}, (name, blk)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", sorted(rsh.CASES))
def test_blocks_equal_oracle(capi, orc, monkeypatch, tmp_path, name, route):
    W, H, C, cuts, ghost, rows, sweeps, _ = rsh.CASES[name]
    set_route(monkeypatch, route)
    traced = ROUTES[route][1]
    paths = []
    factory = traced_factory(capi, monkeypatch, tmp_path, paths) if traced else capi.Grid
    got = rsh.run_intervals(W, H, C, cuts, ghost, sweeps, systems(name), tiling=(8, rows), factory=factory)
    done = 0
    for k, n in enumerate(sweeps):
        done += n
        want = oracle_x(orc, name, done)
        for ch in range(C):
            a, b = got[k][ch].ravel(), want[ch]
            bad = np.flatnonzero(a != b)
            print(f"case {name} route {route} interval {k} channel {ch}: {bad.size} values differ from the oracle"
                  + (f", image rows {bad[0] // W}..{bad[-1] // W}, columns {(bad % W).min()}..{(bad % W).max()}" if bad.size else ""))
            assert np.array_equal(a, b), (name, route, k, ch)
    if traced:
        assert len(paths) == len(cuts) - 1
        check_trace(name, route, paths)


def test_exhausted_ghosts_refuse_until_refreshed(capi, orc, monkeypatch):
    """Case A: 32 sweeps use up 64 ghost rows; two more without halo_refreshed() are refused (CCP_ERR_STATE) and change
    nothing; after the refresh the blocks go on and still give the oracle's bits."""
    name = "A"
    W, H, C, cuts, ghost, rows, sweeps, _ = rsh.CASES[name]
    set_route(monkeypatch, "planner")
    rb = rsh.RowBlocks(W, H, C, cuts, ghost, systems(name), tiling=(8, rows))
    try:
        rb.sweep(32)
        for g in rb.blocks:
            with pytest.raises(capi.CcpError) as e:
                g.sweep(2)
            assert e.value.status == 5
        full = rb.gather()
        assert np.array_equal(full[0].ravel(), oracle_x(orc, name, 32)[0])
        rb.refresh(full)
        rb.sweep(2)
        assert np.array_equal(rb.gather()[0].ravel(), oracle_x(orc, name, 34)[0])
    finally:
        rb.close()
