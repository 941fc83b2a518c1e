"""GPU: unchecked passes that leave out the red half-row store (ccp_grid_fused.hpp, fused_wave STORE_RED = false; the rule
in run_unchecked) give the bits of passes that store both halves (CCP_GS_RED_STORE=1) and of the CPU oracle.  Plans of 1 to
6 passes of mixed depth, odd pass counts, tiny and odd shapes, three channels, Dirichlet-mask grids, several passes per
launch, row blocks with ghosts, the check_every >= 2 path, and every reader of x after a sweep: a stale red half that
leaked out of a call would show in one of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from coursecomputationalphotography_amd import capi
    assert capi.device_count() >= 1
    return capi


def systems(W, H, C):
    from coursecomputationalphotography_amd import synth
    # differently scaled right-hand sides per channel
    return [synth.poisson_system(W, H, 77 + ch)[0] * (10.0 ** (ch - 1)) for ch in range(C)]


def grid(capi, monkeypatch, red_store, W, H, C, bs, tiling=None, multi=False):
    monkeypatch.setenv("CCP_GS_RED_STORE", "1" if red_store else "0")
    monkeypatch.setenv("CCP_GS_MULTI", "1" if multi else "0")
    g = capi.Grid(W, H, C)
    for ch in range(C):
        g.set_b(bs[ch], ch)
    g.fill_x(1.0)
    if tiling:
        g.set_tiling(*tiling)
    return g


def oracle_x(orc, W, H, b, iters):
    import oracle
    from coursecomputationalphotography_amd import synth
    v, c, r = synth.poisson_csr(W, H)
    return orc.multicolour_gauss_seidel(v, c, r, oracle.grid_colour(W, H), b, 0.0, iters)[0]


@pytest.mark.parametrize("W,H,C,iters,tiling", [
    (1, 7, 1, [9], (2, 16)),
    (2, 9, 1, [13], (4, 16)),
    (3, 1, 1, [11], (3, 16)),
    (127, 2, 2, [17], (8, 16)),
    (129, 131, 3, [2, 5, 40], (8, 32)),
    (3 * 96 + 41, 67, 3, [23], (8, 32)),           # not a multiple of the depth-8 strip's 96 useful columns
    (700, 333, 1, [31, 7, 16], (8, 48)),
    (1030, 257, 2, [40], (5, 64)),                 # 8 passes of depth 5
    (300, 301, 1, [3, 4, 6], (2, 16)),             # shallow passes: 2 and 3 passes per call
])
def test_sweeps_equal_full_store_and_oracle(capi, orc, monkeypatch, W, H, C, iters, tiling):
    bs = systems(W, H, C)
    out = {}
    for red_store in (False, True):
        g = grid(capi, monkeypatch, red_store, W, H, C, bs, tiling)
        for n in iters:
            g.sweep(n)
        out[red_store] = [g.get_x(ch).ravel() for ch in range(C)]
        g.close()
    for ch in range(C):
        assert np.array_equal(out[False][ch], out[True][ch]), (W, H, ch)
        assert np.array_equal(out[False][ch], oracle_x(orc, W, H, bs[ch], sum(iters))), (W, H, ch)


@pytest.mark.parametrize("iters", [2, 3, 9, 15, 16, 24, 33, 40])
def test_every_plan_length(capi, orc, monkeypatch, iters):
    W, H, C = 515, 263, 1
    bs = systems(W, H, C)
    got = []
    for red_store in (False, True):
        g = grid(capi, monkeypatch, red_store, W, H, C, bs, (8, 32))
        g.sweep(iters)
        got.append(g.get_x(0).ravel())
        g.close()
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], oracle_x(orc, W, H, bs[0], iters))


@pytest.mark.parametrize("W,H,C,iters,tiling", [
    (1000, 300, 1, [37, 16], (8, 32)),
    (257, 131, 3, [16, 16, 12], (4, 16)),
    (4096, 512, 2, [32, 24], (8, 128)),
])
def test_several_passes_per_launch(capi, orc, monkeypatch, W, H, C, iters, tiling):
    bs = systems(W, H, C)
    out = {}
    for red_store in (False, True):
        g = grid(capi, monkeypatch, red_store, W, H, C, bs, tiling, multi=True)
        for n in iters:
            g.sweep(n)
        g.synchronize()
        out[red_store] = [g.get_x(ch).ravel() for ch in range(C)]
        g.close()
    for ch in range(C):
        assert np.array_equal(out[False][ch], out[True][ch])
        assert np.array_equal(out[False][ch], oracle_x(orc, W, H, bs[ch], sum(iters)))


def test_readers_after_a_sweep(capi, orc, monkeypatch):
    """A sweep, then every reader of x: host copy, residual, a checked solve, the check_every >= 2 path, a second sweep."""
    W, H, C = 777, 389, 3
    bs = systems(W, H, C)
    out = {}
    for red_store in (False, True):
        g = grid(capi, monkeypatch, red_store, W, H, C, bs, (8, 48))
        rec = []
        g.sweep(24)
        rec += [g.get_x(ch).ravel().copy() for ch in range(C)]
        rec += list(np.atleast_1d(g.residual_norm2()[0]))
        g.gauss_seidel(0.0, 11, 1)                     # checked, every sweep
        rec += [g.get_x(ch).ravel().copy() for ch in range(C)]
        g.gauss_seidel(0.0, 20, 4)                     # check_every >= 2: the last pass of each period sums its step
        rec += [g.get_x(ch).ravel().copy() for ch in range(C)]
        g.sweep(17)
        rec += [g.get_x(ch).ravel().copy() for ch in range(C)]
        out[red_store] = rec
        g.close()
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(a, b)
    for ch in range(C):                                # 24 + 11 + 20 + 17 sweeps in all
        assert np.array_equal(out[False][-C + ch], oracle_x(orc, W, H, bs[ch], 72))


def test_masked_grid(capi, monkeypatch):
    from coursecomputationalphotography_amd import synth
    W, H, C = 600, 410, 2
    mask = synth.disc_mask(W, H, seed=99)
    out = {}
    for mode in ("skip", "full", "inplace"):
        monkeypatch.setenv("CCP_GS_RED_STORE", "1" if mode == "full" else "0")
        g = capi.Grid(W, H, C, mask=mask)
        g.randomize_x(4242, 0.0, 255.0)
        g.b_from_x()
        g.fill_x(1.0)
        g.set_tiling(8, 48)
        g.set_fused(mode != "inplace")
        for n in (26, 16, 3):
            g.sweep(n)
        out[mode] = [g.get_x(ch) for ch in range(C)]
        g.close()
    for ch in range(C):
        assert np.array_equal(out["skip"][ch], out["full"][ch])
        assert np.array_equal(out["skip"][ch], out["inplace"][ch])


def test_irregular_region_free_parity(capi, orc, monkeypatch):
    """The CSR entry point's region grid lets a run end in either buffer (odd pass counts, x and x_alt swap)."""
    from coursecomputationalphotography_amd import synth
    mask = synth.disc_mask(300, 220, seed=4321)
    mv, mc, mr, mcol, ys, xs = synth.masked_laplacian_csr(mask)
    mb = synth.csr_apply(mv, mc, mr, synth.x_true(len(ys), 4321))
    got = []
    for red_store in (False, True):
        monkeypatch.setenv("CCP_GS_RED_STORE", "1" if red_store else "0")
        m = capi.CsrMatrix().upload_compressed(mv, mc, mr)
        m.set_colouring(mcol, 2)
        run = []
        for iters in (7, 24, 50):                      # 1, 3 and 7 passes
            run.append(m.gauss_seidel(mb, 0.0, iters, check_every=0)[0])
            assert np.array_equal(run[-1], orc.multicolour_gauss_seidel(mv, mc, mr, mcol, mb, 0.0, iters)[0]), iters
        got.append(run)
        m.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_row_blocks_with_ghosts(capi, monkeypatch):
    """Row blocks with deep ghosts, halos refreshed by hand: the stored row range shrinks from pass to pass."""
    from coursecomputationalphotography_amd import synth
    W, H, iters, ghost = 333, 200, 40, 48
    b, _ = synth.poisson_system(W, H, 11)
    monkeypatch.setenv("CCP_GS_RED_STORE", "1")
    whole = capi.Grid(W, H, 1)
    whole.set_b(b)
    whole.fill_x(1.0)
    whole.sweep(iters)
    want = whole.get_x()
    whole.close()
    monkeypatch.setenv("CCP_GS_RED_STORE", "0")
    cuts = [0, 67, 140, 200]
    blocks = [capi.Grid(W, H, 1, cuts[i], cuts[i + 1] - cuts[i], ghost) for i in range(3)]
    bm = b.reshape(H, W)
    for g in blocks:
        g.set_b(bm[g.first_local_row:g.first_local_row + g.local_rows])
        g.fill_x(1.0)
        g.set_tiling(4, 16)
    done = 0
    while done < iters:
        step = min(ghost // 2, iters - done)            # 24 sweeps between refreshes: six passes of depth 4
        for g in blocks:
            g.sweep(step)
        done += step
        full = np.concatenate([g.get_x_owned() for g in blocks])
        for g in blocks:
            g.set_x(full[g.first_local_row:g.first_local_row + g.local_rows])
            g.halo_refreshed()
    got = np.concatenate([g.get_x_owned() for g in blocks])
    for g in blocks:
        g.close()
    assert np.array_equal(got, want)
