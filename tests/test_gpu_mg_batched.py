"""GPU: the batched channel mode of the multigrid-preconditioned CG (include/ccp_gs.h, CCP_MG_CHANNELS_BATCHED).

The reference is the same handle in sequential mode, and equality is of bits: the raw float64 of x per channel, equal
`iterations` and `converged`, `last_l1_step` equal as bits.  Kinds: structured, mask (disc and blob), weighted Galerkin,
weighted rescaled, rescaled with 10 % fixed pixels (tests/test_gpu_mixed.py's constructions); shapes 1x1 (the one-level
path), 5x3 (the tail directly under level 0), 64x64 and 63x33 (a full six-level tail from 32x32, all 1,365 LDS cells,
and one from a non-square 32x17), 70x40 (two tiles over one tile level, the halo crossing a tile edge),
257x131 (three tile levels, odd sizes, partial edge tiles); C = 1, 2, 3, and 5 once (a second channel group); nu = 2
everywhere, 1 and 4 on 70x40.  Channels that stop at different iterations, the iteration cap across the 16-iteration
batch edge, the mode's handling and what it survives, the refusals (f32, row-block calls, unknown values), tensor_ops
and the C++ facade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mixed_helpers as mh
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG, UNSUPPORTED = 1, 6
KINDS = ["structured", "mask", "galerkin", "rescaled", "rescaled_fixed"]
SHAPES = [(1, 1), (5, 3), (63, 33), (64, 64), (70, 40), (257, 131)]


def weights(W, H, seed):
    """float32 weights in [0.1, 10], lambda = 10 on 1 % of the pixels (and on pixel (0,0): a 1x1 image stays live)."""
    g = mh.rng(seed)
    wx, wy = (g.uniform(0.1, 10.0, (H, W)).astype(np.float32) for _ in range(2))
    lam = np.where(g.uniform(size=(H, W)) < 0.01, 10.0, 0.0).astype(np.float32)
    lam[0, 0] = 10.0
    return wx, wy, lam


def fixed_pixels(W, H, seed):
    fixed = (mh.rng(seed).uniform(size=(H, W)) < 0.1).astype(np.uint8)
    fixed[0, 0] = 0
    return fixed


def handle(kind, W, H, Cn):
    if kind == "structured":
        return capi.Grid(W, H, Cn)
    if kind == "mask":
        return capi.Grid(W, H, Cn, mask=mh.disc_and_blob(W, H))
    wx, wy, lam = weights(W, H, 31 * W + H)
    g = capi.Grid(W, H, Cn, weighted=True)
    if kind != "galerkin":
        g.mg_set_hierarchy("rescaled")
    g.set_weights(wx, wy, lam, fixed=fixed_pixels(W, H, 7 * W + H) if kind == "rescaled_fixed" else None)
    return g


def system(g, seed, scales=None):
    """b = A x* of a random x* in every channel (so b is 0 on dead pixels), channel c scaled by scales[c]; x0 random.
    Returns (bs, x0s) as the handle stores them."""
    g.randomize_x(seed, 0.0, 255.0)
    g.b_from_x()
    bs = [g.get_b(c) for c in range(g.C)]
    if scales is not None:
        bs = [bs[src] * s for src, s in scales]
        for c, b in enumerate(bs):
            g.set_b(b, c)
        bs = [g.get_b(c) for c in range(g.C)]
    g.randomize_x(seed + 1, 0.0, 255.0)
    return bs, [g.get_x(c) for c in range(g.C)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def in_mode(g, mode, x0s, call):
    g.mg_set_channels(mode)
    assert g.mg_channels() == mode
    for c, x in enumerate(x0s):
        g.set_x(x, c)
    out = call(g)
    return out, [g.get_x(c) for c in range(g.C)]


def same_reports(got, want, what):
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.iterations == b.iterations and a.converged == b.converged, (what, c, a.iterations, b.iterations, a.converged, b.converged)
        assert bits(a.last_l1_step) == bits(b.last_l1_step), (what, c, a.last_l1_step, b.last_l1_step)


def same_x(got, want, what):
    for c, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(bits(a), bits(b)), (what, c, float(np.nanmax(np.abs(a - b))))


def both(g, x0s, call, what):
    """call(g) in sequential, then batched, then sequential mode again: the reports and x of the batched run are the
    sequential run's, bit for bit (and the second sequential run's: switching back changes nothing)."""
    ref, xref = in_mode(g, "sequential", x0s, call)
    got, xgot = in_mode(g, "batched", x0s, call)
    again, xagain = in_mode(g, "sequential", x0s, call)
    same_x(xgot, xref, what)
    same_x(xagain, xref, what + " (back)")
    if ref is not None:
        same_reports(got, ref, what)
        same_reports(again, ref, what + " (back)")
    return ref, xref


# ---- 1. the main grid: one V-cycle and the PCG loop ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_batched_equals_sequential(W, H, kind):
    for Cn in (1, 2, 3):
        g = handle(kind, W, H, Cn)
        bs, x0s = system(g, 100 + W + Cn)
        eps = 1e-10 * float(np.linalg.norm(bs[0]))
        both(g, x0s, lambda h: h.mg_apply(2), f"apply {kind} {W}x{H} C={Cn}")
        reps, _ = both(g, x0s, lambda h: h.mg_conjugate_gradient(eps, 40, 2), f"pcg {kind} {W}x{H} C={Cn}")
        print(f"{kind} {W}x{H} C={Cn}: iterations {[r.iterations for r in reps]}, converged {[r.converged for r in reps]}")
        assert all(r.iterations > 0 or r.converged for r in reps)
        g.close()


@pytest.mark.parametrize("kind", ["structured", "galerkin", "rescaled"])
@pytest.mark.parametrize("nu", [1, 4])
def test_other_sweep_counts(nu, kind):
    W, H, Cn = 70, 40, 3
    g = handle(kind, W, H, Cn)
    bs, x0s = system(g, 300 + nu)
    eps = 1e-10 * float(np.linalg.norm(bs[0]))
    both(g, x0s, lambda h: h.mg_apply(nu), f"apply {kind} nu={nu}")
    both(g, x0s, lambda h: h.mg_conjugate_gradient(eps, 40, nu), f"pcg {kind} nu={nu}")
    g.close()


def test_five_channels_make_a_second_group():
    W, H, Cn = 70, 40, 5
    g = handle("rescaled", W, H, Cn)
    bs, x0s = system(g, 500, scales=[(c, 1.0 + c) for c in range(Cn)])
    eps = 1e-10 * float(np.linalg.norm(bs[0]))
    both(g, x0s, lambda h: h.mg_apply(2), "apply C=5")
    reps, xs = both(g, x0s, lambda h: h.mg_conjugate_gradient(eps, 40, 2), "pcg C=5")
    assert all(r.iterations > 0 for r in reps)
    assert not np.array_equal(xs[3], xs[4])
    g.close()


# ---- 2. channels that stop at different iterations -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["structured", "mask", "rescaled", "rescaled_fixed"])
@pytest.mark.parametrize("W,H", [(70, 40), (257, 131)])
def test_channels_stop_on_their_own(W, H, kind):
    """Channel 1's b is 1e-6 x channel 0's (the same absolute epsilon: it stops earlier), channel 2's is 0 (0 iterations,
    converged); all from x = 0."""
    g = handle(kind, W, H, 3)
    bs, x0s = system(g, 700 + W, scales=[(0, 1.0), (0, 1e-6), (0, 0.0)])
    zeros = [np.zeros_like(x) for x in x0s]
    eps = 1e-10 * float(np.linalg.norm(bs[0]))
    reps, xs = both(g, zeros, lambda h: h.mg_conjugate_gradient(eps, 400, 2), f"stops {kind} {W}x{H}")
    its = [r.iterations for r in reps]
    print(f"{kind} {W}x{H}: sequential iterations {its}")
    assert all(r.converged for r in reps), its
    assert its[2] == 0 and 0 < its[1] < its[0], its
    assert not np.any(xs[2])
    # channel 1 starts from the sequential solution of its system, the others from a random x
    start = [x0s[0], xs[1], x0s[2]]
    reps2, _ = both(g, start, lambda h: h.mg_conjugate_gradient(eps, 400, 2), f"solved start {kind} {W}x{H}")
    print(f"{kind} {W}x{H}: from channel 1's solution {[r.iterations for r in reps2]}")
    assert all(r.converged for r in reps2) and reps2[1].iterations <= 1 < reps2[0].iterations
    g.close()


# ---- 3. the caps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["structured", "rescaled"])
def test_iteration_caps(kind):
    W, H, Cn = 70, 40, 3
    g = handle(kind, W, H, Cn)
    _, x0s = system(g, 900, scales=[(0, 1.0), (1, 1e-3), (2, 7.0)])
    reps, _ = both(g, x0s, lambda h: h.mg_conjugate_gradient(0.0, 17, 2), f"cap 17 {kind}")   # across the batch edge at 16
    assert [r.iterations for r in reps] == [17] * Cn and not any(r.converged for r in reps)
    reps, xs = both(g, x0s, lambda h: h.mg_conjugate_gradient(0.0, 0, 2), f"cap 0 {kind}")
    assert [r.iterations for r in reps] == [0] * Cn and not any(r.converged for r in reps)
    same_x(xs, x0s, "cap 0 leaves x alone")
    g.close()


# ---- 4. the mode itself --------------------------------------------------------------------------------------------------
def levels_of(g):
    return [np.stack(t) for t in g.mg_levels()]


@pytest.mark.parametrize("kind", ["structured", "mask", "galerkin"])
def test_default_is_sequential_and_the_round_trip_keeps_its_bits(kind):
    W, H, Cn = 70, 40, 2
    g, ref = handle(kind, W, H, Cn), handle(kind, W, H, Cn)
    value = C.c_int32(-1)
    assert g.L.ccp_grid_mg_get_channels(g.h, C.byref(value)) == 0 and value.value == 0
    assert g.mg_channels() == "sequential"
    bs, x0s = system(g, 40)
    for c in range(Cn):
        ref.set_b(bs[c], c)
    eps = 1e-10 * float(np.linalg.norm(bs[0]))
    g.mg_set_channels("sequential")                          # the current value: nothing happens
    seq_levels = levels_of(g)
    g.mg_set_channels(capi.MG_CHANNELS["batched"])
    assert g.mg_channels() == "batched"
    g.mg_set_channels("batched")
    for a, want in zip(levels_of(g), seq_levels):            # ccp_grid_mg_level: the same bits in both modes
        assert np.array_equal(bits(a), bits(want))
    _, xb = in_mode(g, "batched", x0s, lambda h: h.mg_conjugate_gradient(eps, 30, 2))
    for a, want in zip(levels_of(g), seq_levels):
        assert np.array_equal(bits(a), bits(want))
    g.mg_set_channels("sequential")
    for a, want in zip(levels_of(g), levels_of(ref)):
        assert np.array_equal(bits(a), bits(want))
    rg, xg = in_mode(g, "sequential", x0s, lambda h: h.mg_conjugate_gradient(eps, 30, 2))
    rr, xr = in_mode(ref, "sequential", x0s, lambda h: h.mg_conjugate_gradient(eps, 30, 2))   # never switched
    same_reports(rg, rr, "round trip")
    same_x(xg, xr, "round trip")
    same_x(xb, xr, "batched in between")
    g.close()
    ref.close()


def test_what_the_mode_survives_and_bad_values():
    W, H = 24, 16
    value = C.c_int32(-1)
    g = capi.Grid(W, H, 2, weighted=True)
    for bad in (2, -1, 7):
        assert g.L.ccp_grid_mg_set_channels(g.h, bad) == BAD_ARG
    assert g.L.ccp_grid_mg_get_channels(g.h, None) == BAD_ARG
    assert g.L.ccp_grid_mg_set_channels(None, 1) == BAD_ARG
    assert g.L.ccp_grid_mg_get_channels(None, C.byref(value)) == BAD_ARG
    with pytest.raises(ValueError):
        g.mg_set_channels("interleaved")
    assert g.mg_channels() == "sequential"                   # the refused calls changed nothing
    g.mg_set_channels("batched")                             # before the operator is set
    g.set_weights(*weights(W, H, 1))
    assert g.mg_channels() == "batched"
    g.mg_set_hierarchy("rescaled")
    assert g.mg_channels() == "batched" and g.mg_hierarchy == "rescaled"
    g.set_weights(*weights(W, H, 2), fixed=fixed_pixels(W, H, 3))
    assert g.mg_channels() == "batched"
    g.mg_set_precision("f32")
    assert g.mg_channels() == "batched" and g.mg_precision() == "f32"
    g.mg_set_precision("f64")
    assert g.mg_channels() == "batched"
    bs, x0s = system(g, 11)
    both(g, x0s, lambda h: h.mg_conjugate_gradient(1e-10 * float(np.linalg.norm(bs[0])), 30, 2), "after the setters")
    g.close()
    m = mh.disc_and_blob(40, 30)
    g = capi.Grid(40, 30, 2, mask=m)
    g.mg_set_channels("batched")
    g.set_mask(1 - m)
    assert g.mg_channels() == "batched"
    bs, x0s = system(g, 12)
    both(g, x0s, lambda h: h.mg_conjugate_gradient(1e-10 * float(np.linalg.norm(bs[0])), 30, 2), "after set_mask")
    g.close()


# ---- 5. the refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["channels_first", "precision_first"])
def test_batched_refuses_f32_at_the_solve(order):
    W, H, Cn = 40, 24, 2
    g = handle("rescaled", W, H, Cn)
    bs, x0s = system(g, 21)
    if order == "channels_first":
        g.mg_set_channels("batched")
        g.mg_set_precision("f32")
    else:
        g.mg_set_precision("f32")
        g.mg_set_channels("batched")
    rep = (capi.Report * Cn)()
    assert g.L.ccp_grid_mg_conjugate_gradient(g.h, 1e-6, 10, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply(g.h, 2) == UNSUPPORTED
    for c in range(Cn):
        assert np.array_equal(bits(g.get_x(c)), bits(x0s[c])) and np.array_equal(bits(g.get_b(c)), bits(bs[c]))
    g.mg_set_precision("f64")                                # the handle works again
    reps = g.mg_conjugate_gradient(1e-10 * float(np.linalg.norm(bs[0])), 100)
    assert all(r.converged for r in reps)
    g.close()


def test_rowblocked_calls_refuse_a_batched_handle():
    W, H = 40, 24
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
    g = capi.Grid(W, H, 2)
    _, x0s = system(g, 31)
    g.mg_set_channels("batched")
    g.attach_comm(comm)
    assert g.mg_channels() == "batched"
    rep = (capi.Report * 2)()
    assert g.L.ccp_grid_mg_conjugate_gradient_rowblocked(g.h, 1e-6, 10, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply_rowblocked(g.h, 2) == UNSUPPORTED
    for c in range(2):
        assert np.array_equal(bits(g.get_x(c)), bits(x0s[c]))
    g.mg_set_channels("sequential")
    assert g.L.ccp_grid_mg_apply_rowblocked(g.h, 2) == 0     # the sequential handle is served
    g.attach_comm(None)
    g.close()
    comm.close()
    rb = capi.Grid(20, 10, 1, row_begin=0, row_count=5, ghost=1)   # a handle with ghost rows takes the value ...
    assert rb.L.ccp_grid_mg_set_channels(rb.h, 1) == 0 and rb.mg_channels() == "batched"
    rep = (capi.Report * 1)()
    assert rb.L.ccp_grid_mg_conjugate_gradient_rowblocked(rb.h, 1e-6, 10, 2, rep) == UNSUPPORTED   # ... and is refused at the solve
    assert rb.L.ccp_grid_mg_apply_rowblocked(rb.h, 2) == UNSUPPORTED
    rb.close()


# ---- 6. tensor_ops and the facade ----------------------------------------------------------------------------------------
def test_tensor_ops_batched_equals_sequential(monkeypatch):
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 70, 40, 3
    dev = torch.device("cuda", 0)
    seen = []
    solve = capi.Grid.mg_conjugate_gradient

    def spy(self, *args, **kw):
        seen.append(self.mg_channels())
        return solve(self, *args, **kw)
    monkeypatch.setattr(capi.Grid, "mg_conjugate_gradient", spy)
    gx, gy = (torch.from_numpy(mh.field(W, H, s, -8, 8)[..., None].repeat(Cn, -1) * np.arange(1, Cn + 1, dtype=np.float32)).to(dev)
              for s in (21, 22))
    f = torch.from_numpy(mh.field(W, H, 23, 0.0, 255.0)[..., None].repeat(Cn, -1)).to(dev)
    kw = dict(wx=1.0, wy=1.0, data_weight=0.05, hierarchy="rescaled", out_dtype=torch.float64)
    a = tensor_ops.weighted_solve(gx, gy, f, 200, **kw)
    b = tensor_ops.weighted_solve(gx, gy, f, 200, channels="batched", **kw)
    assert seen == ["sequential", "batched"]
    assert a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))
    img = torch.from_numpy(mh.rng(9).integers(0, 256, (H, W, Cn), dtype=np.uint8)).to(dev)
    a = tensor_ops.wls_smooth(img, 100, hierarchy="rescaled")
    b = tensor_ops.wls_smooth(img, 100, hierarchy="rescaled", channels="batched")
    assert seen[2:] == ["sequential", "batched"] and torch.equal(a, b)
    fixed = torch.from_numpy(mh.ellipse_fixed(W, H)).to(dev)
    a = tensor_ops.constrained_solve(gx, gy, f, f, fixed, 100, data_weight=0.05)
    b = tensor_ops.constrained_solve(gx, gy, f, f, fixed, 100, data_weight=0.05, channels="batched")
    assert torch.equal(a, b)
    a = tensor_ops.seamless_clone_constrained(img, img.flip(0), fixed == 0, 100)
    b = tensor_ops.seamless_clone_constrained(img, img.flip(0), fixed == 0, 100, channels="batched")
    assert torch.equal(a, b)
    a = tensor_ops.solve_channels(gx, gy, [3] * Cn, 100, solver="MultigridConjugateGradient")
    b = tensor_ops.solve_channels(gx, gy, [3] * Cn, 100, solver="MultigridConjugateGradient", channels="batched")
    assert torch.equal(a, b)
    assert seen[4:] == ["sequential", "batched"] * 3
    with pytest.raises(ValueError):
        tensor_ops.weighted_solve(gx, gy, f, 10, data_weight=0.05, channels="interleaved")
    with pytest.raises(ValueError):
        tensor_ops.solve_channels(gx, gy, [3] * Cn, 10, channels="batched")
    with pytest.raises(capi.CcpError) as e:                  # batched + f32: refused at the solve
        tensor_ops.weighted_solve(gx, gy, f, 10, data_weight=0.05, hierarchy="rescaled", precision="f32", channels="batched")
    assert e.value.status == UNSUPPORTED


def test_facade_passes_the_channels_on(tmp_path):
    libdir = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib")
    exe = os.path.join(str(tmp_path), "batched_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "batched_driver.cpp"), "-L" + libdir, "-lccp_gs",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, Cn = 70, 45, 3
    g = mh.rng(31)
    gx, gy = (g.uniform(-8, 8, (H, W, Cn)).astype(np.float32) for _ in range(2))
    f = g.uniform(0.0, 255.0, (H, W, Cn)).astype(np.float32)
    lam = np.full((H, W), 0.1, np.float32)
    fin = os.path.join(str(tmp_path), "w.in")
    arrays = [gx, gy, f, None, None, lam]
    with open(fin, "wb") as fh:
        fh.write(np.array([W, H, Cn] + [a is not None for a in arrays], dtype="<i4").tobytes())
        for a in arrays:
            if a is not None:
                fh.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    outs = {}
    for mode in ("default", "sequential", "batched"):
        fout = os.path.join(str(tmp_path), f"w_{mode}.out")
        p = subprocess.run([exe, mode, "200", fin, fout], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        outs[mode] = np.fromfile(fout, dtype=np.uint8).reshape(H, W, Cn)
    assert np.array_equal(outs["default"], outs["sequential"]) and np.array_equal(outs["batched"], outs["sequential"])
    assert outs["batched"].std() > 0
