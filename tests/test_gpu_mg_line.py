"""GPU: the line smoother of weighted grid handles (include/ccp_gs.h, CCP_MG_SMOOTHER_LINE; csrc/ccp_grid_mgl.hpp).

The reference is tests/line_helpers.py: serial Thomas per line in numpy.  The device solves a line by a partitioned
elimination and cyclic reduction, so its bits differ and one V-cycle is compared in max-norm relative to max |z|.  The
tolerance is 16 x the deviation of the float64 model from the same model carried in np.longdouble on the same system
(computed here, on the CPU): both elimination orders are backward stable on diagonally dominant systems, and the factor
covers the log-depth reduction's constant.  Measured deviations of the model (tests/test_line_helpers.py prints them;
NOTES R18.1 lists them): between 7e-15 (67x3) and 1.3e-13 (257x131) over the shapes below, i.e. bounds between 1.2e-13
and 2.0e-12.  Measured on an MI355X: the device is 5.5e-15 to 1.05e-13 from the model, between 0.4 and 2 times the model's own
deviation, on every shape, nu and hierarchy kind; the PCG counts equal the model's (42, 42, 42; 56; 43).

Shapes: 67x3 (chunk remainder), 1x40 and 40x1 (lines of length 1 in one direction), 257x131 (odd sizes, three line
levels), 2053x9 and 9x2053 (a line longer than one wave's worth of chunks in either direction), 4099x3 and 8200x2 (rows
beyond 4096 cells: 256 lanes with 17 and 33 cells each, longer than kMglChunk, a short last chunk; the model's deviation
there is 6.9e-14 to 8.0e-14 and 3.6e-14 to 5.6e-14, the device 2.3e-14 to 7.1e-14 from the model), 512x384, and 257x131
with fixed pixels (an ellipse's outside, a whole fixed row, a whole fixed column, isolated fixed pixels inside lines).
Weights are the WLS weights of the seeded numpy image, uploaded as the float32 arrays the model reads."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import line_helpers as lh
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG, UNSUPPORTED = 1, 6
SHAPES = [(67, 3, False), (1, 40, False), (40, 1, False), (257, 131, False), (2053, 9, False), (9, 2053, False), (512, 384, False),
          (257, 131, True), (4099, 3, False), (8200, 2, False)]
FACTOR = 16.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def shape_system(W, H, kind, fixed):
    return lh.shape_system(W, H, kind, fixed)


@functools.lru_cache(maxsize=None)
def model_vcycle(W, H, kind, fixed, nu, seed=5):
    """(the float64 model's z, its deviation from the longdouble model)"""
    levels, b = (shape_system(W, H, kind, fixed) if seed == 5 else lh.shape_system(W, H, kind, fixed, seed))[:2]
    dev, z = lh.deviation(levels, b, nu, lh.CS[kind])
    return z, dev


def handle(W, H, kind, fixed, Cn=1):
    _, _, wx, wy, lam, fx = shape_system(W, H, kind, fixed)
    g = capi.Grid(W, H, Cn, weighted=True)
    g.mg_set_hierarchy(kind)
    g.set_weights(wx, wy, lam, fixed=fx)
    return g


# ---- 1. one V-cycle against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["galerkin", "rescaled"])
@pytest.mark.parametrize("W,H,fixed", SHAPES)
def test_vcycle_against_the_model(W, H, fixed, kind):
    levels, b = shape_system(W, H, kind, fixed)[:2]
    g = handle(W, H, kind, fixed)
    g.mg_set_smoother("line")
    assert g.mg_smoother() == "line"
    g.set_b(b)
    for nu in (1, 2):
        want, dev = model_vcycle(W, H, kind, fixed, nu)
        bound = FACTOR * dev
        g.fill_x(123.0)                                          # every cell is written, dead ones with 0
        g.mg_apply(nu)
        got = g.get_x(0)
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{W}x{H}{' fixed' if fixed else ''} {kind} nu={nu}: device vs model {err:.3e}, model vs longdouble {dev:.3e}, bound {bound:.3e}")
        assert np.all(np.isfinite(got))
        assert np.all(got[~levels[0].live] == 0.0)
        assert err <= bound, (W, H, kind, nu, err, bound)
    g.close()


def test_sweeps_zero_is_one_line_sweep_and_two_point_sweeps():
    W, H = 67, 3
    g = handle(W, H, "rescaled", False)
    g.set_b(shape_system(W, H, "rescaled", False)[1])
    out = {}
    for smoother in ("line", "point"):
        g.mg_set_smoother(smoother)
        for nu in (0, 1, 2):
            g.fill_x(0.0)
            g.mg_apply(nu)
            out[smoother, nu] = g.get_x(0)
    assert np.array_equal(bits(out["line", 0]), bits(out["line", 1])) and not np.array_equal(out["line", 0], out["line", 2])
    assert np.array_equal(bits(out["point", 0]), bits(out["point", 2])) and not np.array_equal(out["point", 0], out["point", 1])
    assert g.L.ccp_grid_mg_apply(g.h, 5) == BAD_ARG and g.L.ccp_grid_mg_apply(g.h, -1) == BAD_ARG
    g.close()


# ---- 2. symmetry on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_preconditioner_is_symmetric_on_the_device(fixed):
    W, H, kind = 257, 131, "rescaled"
    levels = shape_system(W, H, kind, fixed)[0]
    g = handle(W, H, kind, fixed)
    g.mg_set_smoother("line")
    rng = np.random.default_rng(17)
    u, v = (np.where(levels[0].live, rng.normal(size=(H, W)), 0.0) for _ in range(2))
    bound = FACTOR * model_vcycle(W, H, kind, fixed, 1)[1]
    out = []
    for vec in (u, v):
        g.set_b(vec)
        g.mg_apply(1)
        out.append(g.get_x(0))
    uMv, vMu = float(np.sum(u * out[1])), float(np.sum(v * out[0]))
    scale = float(np.linalg.norm(u) * np.linalg.norm(v))
    print(f"257x131{' fixed' if fixed else ''}: <u, Mv> - <v, Mu> = {uMv - vMu:.3e}, bound x |u||v| = {bound * scale:.3e}")
    assert abs(uMv - vMu) <= bound * scale, (uMv, vMu, bound * scale)
    g.close()


# ---- 3. the PCG loop ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pcg_case(case):
    """([b per channel], wx, wy, lam, fixed, epsilon, [the model's count per channel])"""
    W, H = (376, 283) if case == "wls_376x283" else (188, 142)
    img = lh.image(W, H)
    wx, wy = lh.wls_weights(img)
    if case.startswith("wls"):
        levels, b = lh.wls_system(W, H)
        lam, fixed = np.ones((H, W), dtype=np.float32), None
        bs = [b]
        if case == "wls_188x142_x3":                             # three channels: three images against the one operator
            bs += [levels[0].lam * lh.image(W, H, seed).astype(np.float64) for seed in (8, 9)]
    else:
        levels, b, fixed = lh.anchor_system(W, H, 16)
        lam, bs = None, [b]
    eps = 1e-10 * float(np.linalg.norm(bs[0]))                   # one epsilon per solve, whatever the channel
    counts = []
    for b in bs:
        _, n, conv, _ = lh.pcg(levels, b, eps, 200, 1, 1.0)
        assert conv
        counts.append(n)
    return bs, wx, wy, lam, fixed, eps, counts


@pytest.mark.parametrize("case", ["wls_188x142_x3", "wls_376x283", "anchors16_188x142"])
def test_pcg_in_line_mode(case):
    bs, wx, wy, lam, fixed, eps, counts = pcg_case(case)
    H, W = bs[0].shape
    g = capi.Grid(W, H, len(bs), weighted=True)
    g.mg_set_hierarchy("rescaled")
    g.set_weights(wx, wy, lam, fixed=fixed)
    for c, b in enumerate(bs):
        g.set_b(b, c)
    results = {}
    for smoother in ("line", "point"):
        g.mg_set_smoother(smoother)
        g.fill_x(0.0)
        reps = g.mg_conjugate_gradient(eps, 400, 0)              # 0: one line sweep, two point sweeps
        rr, _ = g.residual_norm2()
        results[smoother] = [(r.iterations, bool(r.converged)) for r in reps], np.sqrt(rr)
    (line, lrr), (point, _) = results["line"], results["point"]
    print(f"{case}: line {line}, model {counts}, point {point}, |b - A x| {lrr}, epsilon {eps:.3e}")
    for c in range(len(bs)):
        n, conv = line[c]
        assert conv, (case, c, n)
        assert abs(n - counts[c]) <= 1, (case, c, n, counts[c])
        assert lrr[c] < eps, (case, c, lrr[c], eps)
        m, pconv = point[c]
        assert 2 * n <= m, (case, c, n, m, pconv)
    g.close()


# ---- 4. the round trip and what the value survives -----------------------------------------------------------------------
def test_round_trip_keeps_the_point_modes_bits():
    W, H, kind = 257, 131, "rescaled"
    levels, b = shape_system(W, H, kind, True)[:2]
    eps = 1e-8 * float(np.linalg.norm(b))

    def solve(g):
        g.set_b(b)
        g.fill_x(0.0)
        rep = g.mg_conjugate_gradient(eps, 300)[0]
        return g.get_x(0), rep.iterations, rep.converged, rep.last_l1_step

    ref = handle(W, H, kind, True)
    assert ref.mg_smoother() == "point"                          # the default
    want = solve(ref)
    ref.close()
    g = handle(W, H, kind, True)
    g.mg_set_smoother("line")
    g.mg_set_smoother("point")
    got = solve(g)
    g.mg_set_smoother("line")                                    # a line solve in between: its work planes come and go
    mid = solve(g)
    assert mid[2] and mid[1] < want[1]
    g.mg_set_smoother("point")
    again = solve(g)
    for name, out in (("set and unset", got), ("after a line solve", again)):
        assert np.array_equal(bits(out[0]), bits(want[0])), name
        assert out[1:3] == want[1:3] and bits(out[3]) == bits(want[3]), (name, out[1:], want[1:])
    g.close()


def test_what_the_value_survives_and_bad_values():
    W, H = 40, 24
    _, _, wx, wy, lam, _ = shape_system(W, H, "rescaled", False)
    g = capi.Grid(W, H, 2, weighted=True)
    g.mg_set_smoother("line")
    g.set_weights(wx, wy, lam)
    assert g.mg_smoother() == "line"
    g.mg_set_hierarchy("rescaled")
    g.mg_set_precision("f32")
    g.mg_set_channels("batched")
    assert g.mg_smoother() == "line"
    g.mg_set_precision("f64")
    g.mg_set_channels("sequential")
    g.set_weights(wx, wy, lam, fixed=lh.anchors(W, H, 16))
    assert g.mg_smoother() == "line"
    for bad in (2, -1, 7):
        assert g.L.ccp_grid_mg_set_smoother(g.h, bad) == BAD_ARG
    assert g.L.ccp_grid_mg_get_smoother(g.h, None) == BAD_ARG
    assert g.mg_smoother() == "line"
    g.mg_set_smoother(0)
    assert g.mg_smoother() == "point"
    g.close()


# ---- 5. the refusals -----------------------------------------------------------------------------------------------------
def refused(g, rowblocked=False):
    """Both entry points return UNSUPPORTED and leave x and b alone."""
    Cn = g.C
    g.randomize_x(3, 0.0, 255.0)
    g.b_from_x()
    g.randomize_x(4, 0.0, 255.0)
    xs, bs = [g.get_x(c) for c in range(Cn)], [g.get_b(c) for c in range(Cn)]
    rep = (capi.Report * Cn)()
    solve = g.L.ccp_grid_mg_conjugate_gradient_rowblocked if rowblocked else g.L.ccp_grid_mg_conjugate_gradient
    apply = g.L.ccp_grid_mg_apply_rowblocked if rowblocked else g.L.ccp_grid_mg_apply
    assert solve(g.h, 1e-6, 10, 1, rep) == UNSUPPORTED
    assert apply(g.h, 1) == UNSUPPORTED
    for c in range(Cn):
        assert np.array_equal(bits(g.get_x(c)), bits(xs[c])) and np.array_equal(bits(g.get_b(c)), bits(bs[c]))
    return bs


@pytest.mark.parametrize("what", ["structured", "mask", "f32", "f32_first", "batched", "batched_first"])
def test_line_mode_refuses_what_it_does_not_serve(what):
    W, H, Cn = 40, 24, 2
    if what == "structured":
        g = capi.Grid(W, H, Cn)
    elif what == "mask":
        yy, xx = np.mgrid[0:H, 0:W]
        g = capi.Grid(W, H, Cn, mask=((xx - 20) ** 2 + (yy - 12) ** 2 < 100).astype(np.uint8))
    else:
        _, _, wx, wy, lam, _ = shape_system(W, H, "rescaled", False)
        g = capi.Grid(W, H, Cn, weighted=True)
        g.mg_set_hierarchy("rescaled")
        g.set_weights(wx, wy, lam)
    other = {"f32": lambda: g.mg_set_precision("f32"), "batched": lambda: g.mg_set_channels("batched")}.get(what.split("_")[0])
    if what.endswith("_first"):
        other()
        g.mg_set_smoother("line")
    else:
        g.mg_set_smoother("line")
        if other:
            other()
    bs = refused(g)
    g.mg_set_smoother("point")                                   # the handle works again
    reps = g.mg_conjugate_gradient(1e-8 * float(np.linalg.norm(bs[0])), 200)
    assert all(r.converged for r in reps), what
    g.close()


def test_rowblocked_calls_refuse_a_line_handle():
    W, H = 40, 24
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
    g = capi.Grid(W, H, 2)
    g.mg_set_smoother("line")
    g.attach_comm(comm)
    refused(g, rowblocked=True)
    g.mg_set_smoother("point")
    assert g.L.ccp_grid_mg_apply_rowblocked(g.h, 2) == 0         # the point handle is served
    g.attach_comm(None)
    g.close()
    comm.close()
    rb = capi.Grid(20, 10, 1, row_begin=0, row_count=5, ghost=1)   # a handle with ghost rows takes the value ...
    assert rb.L.ccp_grid_mg_set_smoother(rb.h, 1) == 0 and rb.mg_smoother() == "line"
    rep = (capi.Report * 1)()
    assert rb.L.ccp_grid_mg_conjugate_gradient_rowblocked(rb.h, 1e-6, 10, 2, rep) == UNSUPPORTED   # ... and is refused at the solve
    assert rb.L.ccp_grid_mg_apply_rowblocked(rb.h, 2) == UNSUPPORTED
    rb.close()


# ---- 6. tensor_ops and the facade ----------------------------------------------------------------------------------------
def test_tensor_ops_pass_the_smoother_on(monkeypatch):
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 70, 40, 3
    dev = torch.device("cuda", 0)
    seen = []
    solve = capi.Grid.mg_conjugate_gradient

    def spy(self, *args, **kw):
        seen.append(self.mg_smoother())
        return solve(self, *args, **kw)
    monkeypatch.setattr(capi.Grid, "mg_conjugate_gradient", spy)
    rng = np.random.default_rng(21)
    gx, gy = (torch.from_numpy(rng.uniform(-8, 8, (H, W, Cn)).astype(np.float32)).to(dev) for _ in range(2))
    f = torch.from_numpy(rng.uniform(0.0, 255.0, (H, W, Cn)).astype(np.float32)).to(dev)
    kw = dict(wx=1.0, wy=1.0, data_weight=0.05, hierarchy="rescaled", out_dtype=torch.float64)
    a = tensor_ops.weighted_solve(gx, gy, f, 200, **kw)
    b = tensor_ops.weighted_solve(gx, gy, f, 200, smoother="line", **kw)
    assert seen == ["point", "line"]
    assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())       # the same system solved to 1e-10
    img = torch.from_numpy(np.stack([lh.image(W, H, s) for s in (7, 8, 9)], axis=-1)).to(dev)
    a = tensor_ops.wls_smooth(img, 300, hierarchy="rescaled")
    b = tensor_ops.wls_smooth(img, 300, hierarchy="rescaled", smoother="line")
    assert seen[2:] == ["point", "line"]
    assert int((a.to(torch.int16) - b.to(torch.int16)).abs().max()) <= 1
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = torch.from_numpy((((xx - W / 2.0) / (0.45 * W)) ** 2 + ((yy - H / 2.0) / (0.42 * H)) ** 2 > 1.0).astype(np.uint8)).to(dev)
    a = tensor_ops.constrained_solve(gx, gy, f, f, fixed, 200, data_weight=0.05)
    b = tensor_ops.constrained_solve(gx, gy, f, f, fixed, 200, data_weight=0.05, smoother="line")
    assert int((a.to(torch.int16) - b.to(torch.int16)).abs().max()) <= 1
    a = tensor_ops.seamless_clone_constrained(img, img.flip(0), fixed == 0, 200)
    b = tensor_ops.seamless_clone_constrained(img, img.flip(0), fixed == 0, 200, smoother="line")
    assert int((a.to(torch.int16) - b.to(torch.int16)).abs().max()) <= 1
    assert seen[4:] == ["point", "line"] * 2
    with pytest.raises(ValueError):
        tensor_ops.weighted_solve(gx, gy, f, 10, data_weight=0.05, smoother="zebra")
    with pytest.raises(capi.CcpError) as e:                      # line + batched: refused at the solve
        tensor_ops.weighted_solve(gx, gy, f, 10, data_weight=0.05, hierarchy="rescaled", channels="batched", smoother="line")
    assert e.value.status == UNSUPPORTED


def test_facade_passes_the_smoother_on(tmp_path):
    libdir = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib")
    exe = os.path.join(str(tmp_path), "line_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "line_driver.cpp"), "-L" + libdir, "-lccp_gs",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, Cn = 70, 45, 3
    g = np.random.default_rng(31)
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
    for pre in ("", "c_"):                                       # SolveWeighted, then SolveConstrained
        outs = {}
        for mode in ("default", "point", "line"):
            fout = os.path.join(str(tmp_path), f"w_{pre}{mode}.out")
            p = subprocess.run([exe, pre + mode, "200", fin, fout], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, (pre, p.stderr)
            outs[mode] = np.fromfile(fout, dtype=np.uint8).reshape(H, W, Cn)
        assert np.array_equal(outs["default"], outs["point"]), pre
        assert int(np.abs(outs["line"].astype(np.int16) - outs["point"].astype(np.int16)).max()) <= 1, pre
        # Smoother::Line reaches the handle: together with Channels::Batched the solve is refused, which Batched alone is not
        p = subprocess.run([exe, pre + "line_batched", "200", fin, os.path.join(str(tmp_path), "none.out")], capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 2 and "ccp_grid_mg_conjugate_gradient" in p.stderr, (pre, p.returncode, p.stderr)
