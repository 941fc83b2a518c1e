"""GPU: the fp32 V-cycle of the multigrid-preconditioned CG (include/ccp_gs.h, CCP_MG_PRECISION_F32).

A fresh handle reports f64, and a round trip through f32 leaves its levels and its V-cycle bit for bit what a handle
that was never switched gives.  In f32, one V-cycle (nu = 1, 2) equals tests/mixed_helpers.py's float32 V-cycle bit for
bit on structured, mask, weighted (Galerkin, rescaled, rescaled with fixed pixels) handles, on the one-level path (1x1),
the tail directly under level 0 (5x3), a full tail of six levels from 32x32 (64x64: all 1,365 LDS cells) and one whose
first level is not square (63x33: 32x17), two tiles over one tile level (70x40) and three tile levels with odd sizes and
partial edge tiles (257x131).  MG-PCG in f32 takes the model's fp32 count (+-1: the device's dot products are
tree-ordered), converges, leaves an fp64 residual below epsilon, and on the screened system agrees with the f64 mode's x
to 2 epsilon / min lambda.  Channels are independent, bad arguments, row blocks and weights a float cannot hold are
refused, the value survives set_weights / set_mask / mg_set_hierarchy, and tensor_ops and the C++ facade pass it on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import constrained_helpers as ch
import mg_helpers as mg
import mixed_helpers as mh
import rescaled_helpers as rh
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG, UNSUPPORTED = 1, 6
KINDS = ["structured", "mask", "galerkin", "rescaled", "rescaled_fixed"]


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


def handle(kind, W, H, Cn=1):
    """(grid, fp64 model levels, cs) of a handle kind at W x H."""
    if kind == "structured":
        return capi.Grid(W, H, Cn), mg.hierarchy(W, H), 2.0
    if kind == "mask":
        m = mh.disc_and_blob(W, H)
        return capi.Grid(W, H, Cn, mask=m), mg.hierarchy(W, H, m), 2.0
    wx, wy, lam = weights(W, H, 31 * W + H)
    g = capi.Grid(W, H, Cn, weighted=True)
    if kind == "galerkin":
        g.set_weights(wx, wy, lam)
        return g, wh.hierarchy(W, H, wx, wy, lam), 2.0
    g.mg_set_hierarchy("rescaled")
    if kind == "rescaled":
        g.set_weights(wx, wy, lam)
        return g, rh.hierarchy(W, H, wx, wy, lam), 1.0
    fixed = fixed_pixels(W, H, 7 * W + H)
    g.set_weights(wx, wy, lam, fixed=fixed)
    return g, ch.hierarchy(W, H, wx, wy, lam, fixed, "rescaled"), 1.0


def rhs(kind, levels, W, H, seed):
    """b uniform in [-1, 1) (0 outside a mask's region, as the handle stores it)."""
    b = mh.rng(seed).uniform(-1.0, 1.0, (H, W))
    return np.where(levels[0].live, b, 0.0) if kind == "mask" else b


def levels_of(g):
    return [np.stack(t) for t in g.mg_levels()]


# ---- 1. the default, and the round trip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["structured", "mask", "galerkin"])
def test_default_is_f64_and_the_round_trip_keeps_its_bits(kind):
    W, H = 70, 40
    g, levels, _ = handle(kind, W, H)
    ref, _, _ = handle(kind, W, H)
    value = C.c_int32(-1)
    assert g.L.ccp_grid_mg_get_precision(g.h, C.byref(value)) == 0 and value.value == 0
    assert g.mg_precision() == "f64"
    b = rhs(kind, levels, W, H, 5)
    for x in (g, ref):
        x.set_b(b, 0)
    g.mg_set_precision("f64")                                # the current value: nothing happens
    g.mg_set_precision("f32")
    assert g.mg_precision() == "f32"
    g.mg_apply(2)
    in_f32 = g.get_x(0)
    g.mg_set_precision(capi.MG_PRECISIONS["f64"])
    assert g.mg_precision() == "f64"
    for a, want in zip(levels_of(g), levels_of(ref)):
        assert np.array_equal(a, want)
    for nu in (1, 2):
        g.mg_apply(nu)
        ref.mg_apply(nu)
        want = ref.get_x(0)
        assert np.array_equal(g.get_x(0).view(np.uint64), want.view(np.uint64)), nu
    assert not np.array_equal(in_f32, want)                  # the f32 V-cycle did run in between
    g.close()
    ref.close()


# ---- 2. one V-cycle, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (63, 33), (64, 64), (70, 40), (257, 131)])
def test_f32_vcycle_bit_identical(W, H, kind):
    g, levels, cs = handle(kind, W, H)
    g.mg_set_precision("f32")
    levels32 = mh.narrow(levels)
    b = rhs(kind, levels, W, H, 100 + W)
    g.set_b(b, 0)
    for a, lv in zip(g.mg_levels(), levels):                 # ccp_grid_mg_level keeps returning the fp64 coefficients
        for got, want in zip(a, lv.coefficients()):
            assert np.array_equal(got, want)
    for nu in (1, 2):
        g.fill_x(7.0)
        g.mg_apply(nu)
        got, want = g.get_x(0), mh.vcycle(levels32, b, nu, cs)
        assert np.array_equal(got, want), (nu, float(np.abs(got - want).max()))
    g.close()


# ---- 3. MG-PCG ------------------------------------------------------------------------------------------------------------
def pcg_handle(name, W, H):
    """The handle of mixed_helpers.pcg_system(name) with b and x set: (grid, levels, b, x0, cs, min lambda or None)."""
    levels, b, x0, cs, a = mh.pcg_system(name, W, H)
    if name in ("screened", "constrained"):
        g = capi.Grid(W, H, 1, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights(None, None, a["lam"], fixed=a.get("fixed"))
        f3 = [a[k][..., None] for k in ("gx", "gy", "f")]
        if name == "constrained":
            g.assemble_constrained_rhs(*f3, a["v"][..., None], init_x=True)
        else:
            g.assemble_weighted_rhs(*f3, init_x=True)
        assert np.array_equal(g.get_b(0), b) and np.array_equal(g.get_x(0), x0)
        return g, levels, b, x0, cs, float(a["lam"].min())
    g = capi.Grid(W, H, 1, mask=a.get("mask"))
    g.set_b(b, 0)
    g.fill_x(0.0)
    return g, levels, b, x0, cs, None


@pytest.mark.parametrize("name", ["screened", "solve_channel", "mask", "constrained"])
@pytest.mark.parametrize("W,H", [(257, 131), (512, 384)])
def test_f32_pcg_follows_the_model(W, H, name):
    g, levels, b, x0, cs, min_lam = pcg_handle(name, W, H)
    eps = 1e-10 * float(np.linalg.norm(b))
    xs = {}
    for precision in ("f32", "f64"):
        g.mg_set_precision(precision)
        g.set_x(x0, 0)
        rep = g.mg_conjugate_gradient(eps, 200)[0]
        rr, _ = g.residual_norm2()
        print(f"{name} {W}x{H} {precision}: {rep.iterations} iterations, |b - A x| = {np.sqrt(rr[0]):.3e}, epsilon = {eps:.3e}")
        assert rep.converged, (precision, rep.iterations)
        assert rr[0] < eps * eps, (precision, rr[0], eps * eps)
        xs[precision] = g.get_x(0)
        if precision == "f32":
            _, want, conv, _ = mh.pcg(levels, mh.narrow(levels), b, eps, 200, 2, cs, x0)
            print(f"{name} {W}x{H}: the model's fp32 count {want}")
            assert conv and abs(rep.iterations - want) <= 1, (rep.iterations, want)
    if name == "screened":
        diff = float(np.linalg.norm(xs["f32"] - xs["f64"]))
        print(f"{name} {W}x{H}: |x_f32 - x_f64| = {diff:.3e}, bound {2 * eps / min_lam:.3e}")
        assert diff <= 2 * eps / min_lam, (diff, 2 * eps / min_lam)
    g.close()


# ---- 4. channels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["structured", "rescaled"])
def test_f32_channels_are_independent(kind):
    W, H, Cn = 70, 40, 3
    g, levels, _ = handle(kind, W, H, Cn)
    g.mg_set_precision("f32")
    bs = [levels[0].apply(mh.rng(40 + c).uniform(0.0, 255.0, (H, W)) * (1.0 + c)) for c in range(Cn)]
    for c in range(Cn):
        g.set_b(bs[c], c)
    g.fill_x(0.0)
    eps = 1e-10 * max(float(np.linalg.norm(b)) for b in bs)
    reps = g.mg_conjugate_gradient(eps, 100)
    assert all(r.converged for r in reps), [r.iterations for r in reps]
    for c in range(Cn):
        one, _, _ = handle(kind, W, H, 1)
        one.mg_set_precision("f32")
        one.set_b(bs[c], 0)
        one.fill_x(0.0)
        rep = one.mg_conjugate_gradient(eps, 100)[0]
        assert rep.converged and rep.iterations == reps[c].iterations
        assert np.array_equal(one.get_x(0).view(np.uint64), g.get_x(c).view(np.uint64)), c
        one.close()
    g.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_and_what_the_value_survives():
    W, H = 24, 16
    value = C.c_int32(-1)
    g = capi.Grid(W, H, 1, weighted=True)
    for bad in (2, -1, 7):
        assert g.L.ccp_grid_mg_set_precision(g.h, bad) == BAD_ARG
    assert g.L.ccp_grid_mg_get_precision(g.h, None) == BAD_ARG
    assert g.L.ccp_grid_mg_set_precision(None, 1) == BAD_ARG
    assert g.L.ccp_grid_mg_get_precision(None, C.byref(value)) == BAD_ARG
    with pytest.raises(ValueError):
        g.mg_set_precision("f16")
    assert g.mg_precision() == "f64"                         # the refused calls changed nothing
    g.mg_set_precision("f32")                                # before the operator is set
    g.set_weights(*weights(W, H, 1))
    assert g.mg_precision() == "f32"
    g.mg_set_hierarchy("rescaled")
    assert g.mg_precision() == "f32" and g.mg_hierarchy == "rescaled"
    g.set_weights(*weights(W, H, 2), fixed=fixed_pixels(W, H, 3))
    assert g.mg_precision() == "f32"
    g.close()
    m = mh.disc_and_blob(40, 30)
    g = capi.Grid(40, 30, 1, mask=m)
    g.mg_set_precision("f32")
    g.set_mask(1 - m)
    assert g.mg_precision() == "f32"
    g.close()
    rb = capi.Grid(20, 10, 1, row_begin=0, row_count=5, ghost=1)
    assert rb.L.ccp_grid_mg_set_precision(rb.h, capi.MG_PRECISIONS["f32"]) == UNSUPPORTED
    assert rb.L.ccp_grid_mg_set_precision(rb.h, capi.MG_PRECISIONS["f64"]) == 0
    assert rb.mg_precision() == "f64"
    rb.close()


def test_rowblocked_calls_refuse_f32_on_a_whole_image():
    """A whole-image handle on a world-1 communicator is the one way to hold f32 and reach the row-block calls."""
    W, H = 40, 24
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
    g = capi.Grid(W, H, 1)
    g.randomize_x(5, 0.0, 255.0)
    g.b_from_x()
    g.randomize_x(6, 0.0, 255.0)
    x0 = g.get_x(0)
    g.mg_set_precision("f32")
    g.attach_comm(comm)
    assert g.mg_precision() == "f32"
    rep = (capi.Report * 1)()
    assert g.L.ccp_grid_mg_conjugate_gradient_rowblocked(g.h, 1e-6, 10, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply_rowblocked(g.h, 2) == UNSUPPORTED
    assert np.array_equal(g.get_x(0).view(np.uint64), x0.view(np.uint64))
    g.attach_comm(None)
    g.close()
    comm.close()


def test_weights_a_float_cannot_hold_are_refused_at_the_solve():
    W, H = 24, 16
    big = np.full((H, W), 3e38, np.float32)                  # float32-finite, but d = lambda + the edge weights is not
    g = capi.Grid(W, H, 1, weighted=True)
    g.set_weights(big, big, big)
    g.randomize_x(3, 0.0, 255.0)
    g.b_from_x()
    g.randomize_x(4, 0.0, 255.0)
    b, x0 = g.get_b(0), g.get_x(0)
    g.mg_set_precision("f32")
    rep = (capi.Report * 1)()
    assert g.L.ccp_grid_mg_conjugate_gradient(g.h, 1e-10 * float(np.linalg.norm(b)), 50, 2, rep) == UNSUPPORTED
    assert g.L.ccp_grid_mg_apply(g.h, 2) == UNSUPPORTED
    assert np.array_equal(g.get_x(0).view(np.uint64), x0.view(np.uint64)) and np.array_equal(g.get_b(0).view(np.uint64), b.view(np.uint64))
    assert len(g.mg_levels()) == len(wh.hierarchy(W, H))     # the fp64 coefficients are still there to look at
    g.mg_set_precision("f64")
    r = g.mg_conjugate_gradient(1e-10 * float(np.linalg.norm(b)), 50)[0]
    assert r.converged
    g.close()


# ---- 6. tensor_ops and the facade -----------------------------------------------------------------------------------------
def test_tensor_ops_pass_the_precision_on(monkeypatch):
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 64, 48, 3
    dev = torch.device("cuda", 0)
    seen = []
    solve = capi.Grid.mg_conjugate_gradient

    def spy(self, *args, **kw):
        seen.append(self.mg_precision())
        return solve(self, *args, **kw)
    monkeypatch.setattr(capi.Grid, "mg_conjugate_gradient", spy)
    gx, gy = (torch.from_numpy(mh.field(W, H, s, -8, 8)[..., None].repeat(Cn, -1)).to(dev) for s in (21, 22))
    f = torch.from_numpy(mh.field(W, H, 23, 0.0, 255.0)[..., None].repeat(Cn, -1)).to(dev)
    kw = dict(wx=1.0, wy=1.0, data_weight=0.05, hierarchy="rescaled")
    a = tensor_ops.weighted_solve(gx, gy, f, 200, **kw)
    b = tensor_ops.weighted_solve(gx, gy, f, 200, precision="f32", **kw)
    assert seen == ["f64", "f32"]
    assert a.dtype == torch.uint8 and (a.to(torch.int16) - b.to(torch.int16)).abs().max().item() <= 1
    img = torch.from_numpy(mh.rng(9).integers(0, 256, (H, W, Cn), dtype=np.uint8)).to(dev)
    a = tensor_ops.wls_smooth(img, 200, hierarchy="rescaled")
    b = tensor_ops.wls_smooth(img, 200, hierarchy="rescaled", precision="f32")
    assert seen[2:] == ["f64", "f32"]
    assert (a.to(torch.int16) - b.to(torch.int16)).abs().max().item() <= 1
    fixed = torch.from_numpy(mh.ellipse_fixed(W, H)).to(dev)
    tensor_ops.constrained_solve(gx, gy, f, f, fixed, 200, data_weight=0.05, precision="f32")
    tensor_ops.seamless_clone_constrained(img, img.flip(0), fixed == 0, 200, precision="f32")
    tensor_ops.solve_channels(gx, gy, [3] * Cn, 200, solver="MultigridConjugateGradient", precision="f32")
    tensor_ops.solve_channels(gx, gy, [3] * Cn, 200, solver="MultigridConjugateGradient")
    assert seen[4:] == ["f32", "f32", "f32", "f64"]
    with pytest.raises(ValueError):
        tensor_ops.weighted_solve(gx, gy, f, 10, data_weight=0.05, precision="f16")
    with pytest.raises(ValueError):
        tensor_ops.solve_channels(gx, gy, [3] * Cn, 10, precision="f32")


def run_driver(exe, tmp_path, precision, iterations, W, H, Cn, arrays, expect=0):
    fin, fout = os.path.join(str(tmp_path), "w.in"), os.path.join(str(tmp_path), f"w_{precision}.out")
    with open(fin, "wb") as fh:
        fh.write(np.array([W, H, Cn] + [a is not None for a in arrays], dtype="<i4").tobytes())
        for a in arrays:
            if a is not None:
                fh.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    p = subprocess.run([exe, precision, str(iterations), fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == expect, p.stderr
    return np.fromfile(fout, dtype=np.uint8).reshape(H, W, Cn) if expect == 0 else p.stderr


def test_facade_passes_the_precision_on(tmp_path):
    libdir = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib")
    exe = os.path.join(str(tmp_path), "mixed_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "mixed_driver.cpp"), "-L" + libdir, "-lccp_gs",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, Cn = 70, 45, 3
    g = mh.rng(31)
    gx, gy = (g.uniform(-8, 8, (H, W, Cn)).astype(np.float32) for _ in range(2))
    f = g.uniform(0.0, 255.0, (H, W, Cn)).astype(np.float32)
    lam = np.full((H, W), 0.1, np.float32)
    outs = {k: run_driver(exe, tmp_path, k, 200, W, H, Cn, [gx, gy, f, None, None, lam]) for k in ("default", "double", "single")}
    assert np.array_equal(outs["default"], outs["double"])
    assert np.abs(outs["single"].astype(np.int16) - outs["default"].astype(np.int16)).max() <= 1
    # weights a float cannot hold: only a call that really runs the float V-cycle refuses them
    big = np.full((H, W), 3e38, np.float32)
    run_driver(exe, tmp_path, "double", 50, W, H, Cn, [None, None, f, big, big, big])
    err = run_driver(exe, tmp_path, "single", 50, W, H, Cn, [None, None, f, big, big, big], expect=2)
    assert "ccp_grid_mg_conjugate_gradient" in err, err
