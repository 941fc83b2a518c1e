"""GPU: hard constraints (fixed pixels) on weighted grid handles (include/ccp_gs.h, "Hard constraints on weighted grids").

Bit for bit against tests/constrained_helpers.py: every level of both hierarchy kinds, b, x after the assembly (init on
and off), b := A x, the residual and one V-cycle (nu = 1..4), on random weights with a random 30 % of the pixels fixed and
on the special sets (none, all, the frame, an enclosed free pixel, two adjacent fixed pixels); an empty set equals the
unconstrained calls on the same handle.  The device twins equal the host twins for every mask and value dtype and
layout.  MG-PCG converges on a region that reaches the canvas border, to the model's iteration count (+-1) and to 1e-6
of scipy's direct solve, and leaves the fixed pixels bit for bit.  tensor_ops and the C++ facade solve the same systems;
the refusals mirror the weighted calls'."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi
import scipy.sparse.linalg as sla
import torch

import constrained_helpers as ch
import per_channel_helpers as pch
import test_gpu_weighted as tgw
import weighted_helpers as wh
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

ROOT = tgw.ROOT
BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
KINDS = ("galerkin", "rescaled")
rng, field, random_weights = tgw.rng, tgw.field, tgw.random_weights


def levels_equal(grid, levels, what=""):
    got = grid.mg_levels()
    assert len(got) == len(levels)
    for k, ((d, we, ws), lv) in enumerate(zip(got, levels)):
        assert np.array_equal(d, lv.d), f"{what} level {k}: diagonal"
        assert np.array_equal(we, lv.we), f"{what} level {k}: east weights"
        assert np.array_equal(ws, lv.ws), f"{what} level {k}: south weights"


def random_fixed(W, H, seed, share=0.3):
    return (rng(seed).uniform(size=(H, W)) < share).astype(np.uint8)


def special_fixed(name, W, H):
    m = np.zeros((H, W), np.uint8)
    cy, cx = H // 2, W // 2
    if name == "all":
        m[:] = 1
    elif name == "frame":
        m[0, :] = m[-1, :] = 1
        m[:, 0] = m[:, -1] = 1
    elif name == "enclosed":                               # a free pixel all of whose neighbours are fixed
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= cy + dy < H and 0 <= cx + dx < W:
                m[cy + dy, cx + dx] = 1
    elif name == "pair":                                   # two adjacent fixed pixels
        m[cy, cx] = 1
        if W > 1:
            m[cy, (cx + 1) % W] = 1
        else:
            m[(cy + 1) % H, cx] = 1
    else:
        assert name == "none"
    return m


def check_against_helper(W, H, Cn, fixed, seed):
    """One handle through every comparison of the module docstring's first paragraph."""
    wx, wy, lam = random_weights(W, H, seed)
    gx, gy, f = field(W, H, Cn, seed + 1), field(W, H, Cn, seed + 2), field(W, H, Cn, seed + 3, 0.0, 255.0)
    v = field(W, H, Cn, seed + 4, -20.0, 300.0)
    xs = [rng(seed + 5 + c).uniform(-100, 100, (H, W)) for c in range(Cn)]
    g = capi.Grid(W, H, Cn, weighted=True)
    g.set_weights(wx, wy, lam, fixed=fixed)
    hier = {kind: ch.hierarchy(W, H, wx, wy, lam, fixed, kind) for kind in KINDS}
    lv = hier["galerkin"][0]
    assert g.constraint_info() == ch.counts(lv)
    for kind in KINDS:
        g.mg_set_hierarchy(kind)
        levels_equal(g, hier[kind], kind)
    bs = [ch.rhs(lv, gx[..., c], gy[..., c], f[..., c], v[..., c]) for c in range(Cn)]
    for init in (False, True):
        for c in range(Cn):
            g.set_x(xs[c], c)
        g.set_b(np.full((H, W), 7.0), 0)
        g.assemble_constrained_rhs(gx, gy, f, v, init_x=init)
        for c in range(Cn):
            assert np.array_equal(g.get_b(c), bs[c]), f"b, channel {c}, init {init}"
            assert np.array_equal(g.get_x(c), ch.x_after(lv, xs[c], f[..., c], v[..., c], init)), f"x, channel {c}, init {init}"
    # the weighted call on this operator: the constrained one with values = 0, guidance on the original weights
    g.assemble_weighted_rhs(gx, gy, f, init_x=True)
    for c in range(Cn):
        assert np.array_equal(g.get_b(c), ch.rhs(lv, gx[..., c], gy[..., c], f[..., c], None)), f"values NULL, channel {c}"
        assert np.array_equal(g.get_x(c), ch.x_after(lv, xs[c], f[..., c], None, True))
    # b := A x and the residual: fixed pixels are dead
    for c in range(Cn):
        g.set_x(xs[c], c)
    g.b_from_x()
    for c in range(Cn):
        assert np.array_equal(g.get_b(c), lv.apply(xs[c])), f"A x, channel {c}"
    rr, _ = g.residual_norm2()
    assert np.all(rr == 0.0)
    for kind in KINDS:
        g.mg_set_hierarchy(kind)
        for nu in (1, 2, 3, 4):
            for c in range(Cn):
                g.set_b(bs[c], c)
            g.mg_apply(nu)
            for c in range(Cn):
                assert np.array_equal(g.get_x(c), ch.vcycle(hier[kind], bs[c], nu, kind)), f"{kind} nu {nu}, channel {c}"
    g.close()


# ---- 1. bit for bit against the helper ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("W,H", tgw.BIT_SHAPES)
def test_random_fixed_pixels_bit_identical(W, H, Cn):
    check_against_helper(W, H, Cn, random_fixed(W, H, 31 + W * H), 2000 + W * H)


@pytest.mark.parametrize("name", ["none", "all", "frame", "enclosed", "pair"])
@pytest.mark.parametrize("W,H,Cn", [(1, 1, 1), (5, 1, 3), (1, 5, 1), (3, 6, 3), (65, 31, 3), (130, 5, 1)])
def test_special_sets_bit_identical(W, H, Cn, name):
    check_against_helper(W, H, Cn, special_fixed(name, W, H), 3000 + W * H)


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("W,H", tgw.BIT_SHAPES)
def test_empty_set_equals_the_unconstrained_calls(W, H, Cn):
    wx, wy, lam = random_weights(W, H, 4000 + W * H)
    gx, gy, f = field(W, H, Cn, 1), field(W, H, Cn, 2), field(W, H, Cn, 3, 0.0, 255.0)
    v = field(W, H, Cn, 4, 0.0, 255.0)
    g = capi.Grid(W, H, Cn, weighted=True)
    got = {}
    for how in ("plain", "empty mask"):
        g.set_weights(wx, wy, lam, fixed=None if how == "plain" else np.zeros((H, W), np.uint8))
        for kind in KINDS:
            g.mg_set_hierarchy(kind)
            got[how, kind] = g.mg_levels()
        g.fill_x(3.0)
        if how == "plain":
            g.assemble_weighted_rhs(gx, gy, f, init_x=True)
        else:
            g.assemble_constrained_rhs(gx, gy, f, v, init_x=True)
        got[how, "b"] = [g.get_b(c) for c in range(Cn)]
        got[how, "x"] = [g.get_x(c) for c in range(Cn)]
        g.mg_apply(2)
        got[how, "z"] = [g.get_x(c) for c in range(Cn)]
        got[how, "info"] = g.constraint_info()
    lv = wh.hierarchy(W, H, wx, wy, lam)[0]
    assert got["plain", "info"] == got["empty mask", "info"] == (0, int(lv.live.sum()), 0)
    for kind in KINDS:
        for a, b in zip(got["plain", kind], got["empty mask", kind]):
            for p, q in zip(a, b):
                assert np.array_equal(p, q), kind
    for key in ("b", "x", "z"):
        for c in range(Cn):
            assert np.array_equal(got["plain", key][c], got["empty mask", key][c]), (key, c)
    for c in range(Cn):
        assert np.array_equal(got["plain", "b"][c], wh.rhs(lv, gx[..., c], gy[..., c], f[..., c]))
    g.close()


# ---- 2. device twins ---------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def state(g):
    return [g.mg_levels()] + [[g.get_b(c) for c in range(g.C)], [g.get_x(c) for c in range(g.C)], g.constraint_info()]


def states_equal(a, b, what):
    for la, lb in zip(a[0], b[0]):
        for p, q in zip(la, lb):
            assert np.array_equal(p, q), what
    for ka in (1, 2):
        for p, q in zip(a[ka], b[ka]):
            assert np.array_equal(p, q), (what, "b" if ka == 1 else "x")
    assert a[3] == b[3], what


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 7), (65, 31), (257, 131)])
def test_device_twins_equal_host_twins(W, H, Cn):
    wx, wy, lam = random_weights(W, H, 77 + W)
    fixed = random_fixed(W, H, 5 + W)
    gx, gy = field(W, H, Cn, 1), field(W, H, Cn, 2)
    f8 = rng(3).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    v8 = rng(4).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    x0 = rng(6).uniform(-9, 9, (H, W))
    host = capi.Grid(W, H, Cn, weighted=True)
    host.set_weights(wx, wy, lam, fixed=fixed)
    want = {}
    for init in (False, True):
        for c in range(Cn):
            host.set_x(x0, c)
        host.assemble_constrained_rhs(gx, gy, f8.astype(np.float32), v8.astype(np.float32), init_x=init)
        want[init] = state(host)
    host.close()
    tw = [torch.from_numpy(a).to(DEV) for a in (wx, wy, lam)]
    tgx, tgy = torch.from_numpy(gx).to(DEV), torch.from_numpy(gy).to(DEV)
    tf, tv, tm = torch.from_numpy(f8).to(DEV), torch.from_numpy(v8).to(DEV), torch.from_numpy(fixed).to(DEV)
    big = torch.full((H + 5, W + 9), 1, dtype=torch.uint8, device=DEV)
    big[2:2 + H, 3:3 + W] = tm
    planar = tv.permute(2, 0, 1).contiguous().permute(1, 2, 0)            # C x H x W storage
    masks = {"u8": tm, "bool": tm != 0, "f32": tm.to(torch.float32) * -2.5, "f64": tm.to(torch.float64) * 1e-300,
             "window": big[2:2 + H, 3:3 + W], "transposed": tm.t().contiguous().t()}
    values = {"u8": tv, "f32": tv.to(torch.float32), "f64": tv.to(torch.float64), "planar": planar,
              "planar f64": planar.to(torch.float64)}
    d = capi.Grid(W, H, Cn, weighted=True)
    for mname, m in masks.items():
        d.set_weights_tensor(*tw, fixed=m)
        for vname, val in (values.items() if mname == "u8" else [("u8", tv)]):
            for init in (False, True):
                for c in range(Cn):
                    d.set_x(x0, c)
                d.assemble_constrained_rhs_tensor(tgx, tgy, tf.to(val.dtype), val, init_x=init)
                torch.cuda.current_stream().synchronize()
                states_equal(state(d), want[init], (mname, vname, init))
    d.close()


RHS_DTYPES = (None, "u8", "f32", "f64")


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("W,H", [(9, 7), (257, 5)])        # odd both ways; a second block in x that holds one pixel
def test_every_dtype_pair_of_f_and_values(W, H, per_channel):
    """The dtypes of f and of values are run-time fields of the right-hand-side kernel's views: every pair from
    {absent, u8, f32, f64}^2 with gx, gy present, with and without init, on a shared operator with a random mask and on
    one operator per channel with a mask per channel.  f and values are integers in [0, 255], so every dtype carries
    the same numbers and one reference per (f present, values present, init) serves all pairs: b and x bit for bit."""
    Cn = 3
    gx, gy = field(W, H, Cn, 1), field(W, H, Cn, 2)
    f8 = rng(3).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    v8 = rng(4).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    x0 = [rng(6 + c).uniform(-9, 9, (H, W)) for c in range(Cn)]
    zero = np.zeros((H, W, Cn), np.float32)
    g = capi.Grid(W, H, Cn, weighted=True)
    if per_channel:
        ws = [random_weights(W, H, 80 + W + c) for c in range(Cn)]
        wx, wy, lam = (np.stack([w[i] for w in ws], axis=-1) for i in range(3))
        fixed = np.stack([random_fixed(W, H, 9 + W + c) for c in range(Cn)], axis=-1)
        assert all(fixed[..., c].any() for c in range(Cn))
        g.set_weights_per_channel_tensor(*[torch.from_numpy(a).to(DEV) for a in (wx, wy, lam, fixed)])
        lv = [pch.channel_levels((wx, wy, lam, fixed), c)[0] for c in range(Cn)]
    else:
        wx, wy, lam = random_weights(W, H, 77 + W)
        fixed = random_fixed(W, H, 5 + W)
        g.set_weights_tensor(*[torch.from_numpy(a).to(DEV) for a in (wx, wy, lam)], fixed=torch.from_numpy(fixed).to(DEV))
        lv = [ch.level0(W, H, wx, wy, lam, fixed)] * Cn
    want = {}
    for hf in (False, True):
        for hv in (False, True):
            ins = (gx, gy, f8 if hf else zero, v8 if hv else zero)            # an absent input reads 0
            b = [pch.channel_rhs([lv[c]], ins, c) if per_channel else ch.rhs(lv[c], gx[..., c], gy[..., c], ins[2][..., c], ins[3][..., c])
                 for c in range(Cn)]
            for init in (False, True):
                want[hf, hv, init] = (b, [ch.x_after(lv[c], x0[c], ins[2][..., c], ins[3][..., c], init) for c in range(Cn)])
    tgx, tgy = torch.from_numpy(gx).to(DEV), torch.from_numpy(gy).to(DEV)
    to = {None: lambda a: None, "u8": lambda a: torch.from_numpy(a).to(DEV), "f32": lambda a: torch.from_numpy(a).to(DEV).to(torch.float32),
          "f64": lambda a: torch.from_numpy(a).to(DEV).to(torch.float64)}
    for fd in RHS_DTYPES:
        for vd in RHS_DTYPES:
            for init in (False, True):
                for c in range(Cn):
                    g.set_x(x0[c], c)
                    g.set_b(np.full((H, W), 7.0), c)
                g.assemble_constrained_rhs_tensor(tgx, tgy, to[fd](f8), to[vd](v8), init_x=init)
                torch.cuda.current_stream().synchronize()
                b, x = want[fd is not None, vd is not None, init]
                for c in range(Cn):
                    assert np.array_equal(g.get_b(c), b[c]), ("b", fd, vd, init, c)
                    assert np.array_equal(g.get_x(c), x[c]), ("x", fd, vd, init, c)
    g.close()


def test_broadcast_mask_and_values():
    """A stride-0 mask (one row for every row) and stride-0 values (one colour for every pixel)."""
    W, H, Cn = 65, 31, 3
    wx, wy, lam = random_weights(W, H, 9)
    row = (rng(8).uniform(size=W) < 0.3).astype(np.uint8)
    colour = np.array([12.5, 200.0, 77.25])
    gx, gy, f = field(W, H, Cn, 1), field(W, H, Cn, 2), field(W, H, Cn, 3, 0.0, 255.0)
    host = capi.Grid(W, H, Cn, weighted=True)
    host.set_weights(wx, wy, lam, fixed=np.broadcast_to(row, (H, W)))
    host.assemble_constrained_rhs(gx, gy, f, np.broadcast_to(colour.astype(np.float32), (H, W, Cn)), init_x=True)
    d = capi.Grid(W, H, Cn, weighted=True)
    d.set_weights_tensor(*[torch.from_numpy(a).to(DEV) for a in (wx, wy, lam)], fixed=torch.from_numpy(row).to(DEV).expand(H, W))
    d.assemble_constrained_rhs_tensor(*[torch.from_numpy(a).to(DEV) for a in (gx, gy, f)],
                                      torch.from_numpy(colour).to(DEV).expand(H, W, Cn), init_x=True)
    torch.cuda.current_stream().synchronize()
    states_equal(state(d), state(host), "broadcast")
    assert d.constraint_info()[0] == int(row.sum()) * H
    host.close()
    d.close()


def test_stream_ordered_without_host_sync():
    """assemble -> composite on a non-default torch stream, the inputs produced by torch kernels on that stream just
    before: no host synchronisation until the end, the result equals the host route."""
    W, H, Cn = 1537, 1031, 3
    lam = np.full((H, W), 0.05, np.float32)
    fixed = random_fixed(W, H, 12, 0.4)
    gx, gy, f = field(W, H, Cn, 1), field(W, H, Cn, 2), field(W, H, Cn, 3, 0.0, 255.0)
    v = rng(4).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    host = capi.Grid(W, H, Cn, weighted=True)
    host.set_weights(None, None, lam, fixed=fixed)
    host.assemble_constrained_rhs(gx, gy, f, v.astype(np.float32), init_x=True)
    want_u8, want_b = host.store_u8(), np.stack([host.get_b(c) for c in range(Cn)], axis=-1)
    host.close()
    dev = capi.Grid(W, H, Cn, weighted=True)
    dev.set_weights_tensor(None, None, torch.from_numpy(lam).to(DEV), fixed=torch.from_numpy(fixed).to(DEV))   # synchronises: the verdict
    s = torch.cuda.Stream(device=DEV)
    staged = [torch.from_numpy(a).pin_memory() for a in (gx, gy, f, v)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        tgx, tgy, tf, tv = (t.to(DEV, non_blocking=True) for t in staged)
        tgx = (tgx * 2.0) * 0.5                                      # torch kernels on s write the inputs
        tv = tv + 0
        dev.assemble_constrained_rhs_tensor(tgx, tgy, tf, tv, init_x=True)
        out = dev.store_u8_tensor()
        b = dev.get_b_tensor()
        res, resb = out.to("cpu", non_blocking=True), b.to("cpu", non_blocking=True)
    torch.cuda.synchronize()
    assert np.array_equal(res.numpy(), want_u8) and np.array_equal(resb.numpy(), want_b)
    dev.close()


# ---- 3. solves -----------------------------------------------------------------------------------------------------------
def region(W, H, seed=5):
    """Fixed = outside an ellipse that reaches the left and right canvas borders, plus a random 0.5 % of the pixels, plus
    one pixel of every connected free component (lambda = 0 stays non-singular)."""
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = ((xx - (W - 1) / 2) / (0.55 * W)) ** 2 + ((yy - (H - 1) / 2) / (0.35 * H)) ** 2 >= 1.0
    assert not fixed[H // 2, 0] and not fixed[H // 2, W - 1] and fixed[0, 0]
    fixed |= rng(seed).uniform(size=(H, W)) < 0.005
    labels, n = ndi.label(~fixed)
    for k in range(1, n + 1):
        fixed.ravel()[np.flatnonzero(labels.ravel() == k)[0]] = True
    return fixed.astype(np.uint8)


def solve_systems(W, H):
    yield "poisson", None, None, None
    for name, wx, wy, lam in tgw.systems(W, H):
        if name != "data_only":
            yield name, wx, wy, lam


SYSTEM_NAMES = ["poisson", "screened_1e-3", "screened_1", "screened_100", "wls"]


@pytest.mark.parametrize("name", SYSTEM_NAMES)
@pytest.mark.parametrize("W,H", [(257, 131), (512, 512)])
def test_pcg_on_a_region_touching_the_border(W, H, name):
    _, wx, wy, lam = next(s for s in solve_systems(W, H) if s[0] == name)
    fixed = region(W, H)
    gx, gy, f = field(W, H, 1, 1), field(W, H, 1, 2), field(W, H, 1, 3, 0.0, 255.0)
    v = field(W, H, 1, 4, -30.0, 290.0)
    A_ff, b_f, free = ch.free_system(W, H, wx, wy, lam, fixed, gx[..., 0], gy[..., 0], f[..., 0], v[..., 0])
    want = sla.spsolve(A_ff.tocsc(), b_f)
    g = capi.Grid(W, H, 1, weighted=True)
    g.set_weights(wx, wy, lam, fixed=fixed)
    for kind in KINDS:
        g.mg_set_hierarchy(kind)
        g.assemble_constrained_rhs(gx, gy, f, v, init_x=True)
        b, x0 = g.get_b(0), g.get_x(0)
        eps = 1e-10 * float(np.linalg.norm(b))
        rep = g.mg_conjugate_gradient(eps, 300)[0]
        print(f"{W}x{H} {name} {kind}: {rep.iterations} iterations, converged {rep.converged}")
        assert rep.converged, (name, kind, rep.iterations)
        x = g.get_x(0)
        err = np.abs(x.ravel()[free] - want).max()
        assert err <= 1e-6 * np.abs(want).max(), (name, kind, rep.iterations, err)
        assert np.array_equal(x[fixed != 0], v[..., 0].astype(np.float64)[fixed != 0]), (name, kind)
        assert np.array_equal(g.store_u8()[..., 0], np.clip(x, 0.0, 255.0).astype(np.uint8)), (name, kind)
        if (W, H) == (257, 131):
            levels = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
            assert np.array_equal(b, ch.rhs(levels[0], gx[..., 0], gy[..., 0], f[..., 0], v[..., 0]))
            xm, its, conv, _ = ch.pcg(levels, b, eps, 300, 2, x0, kind)
            print(f"{W}x{H} {name} {kind}: the model's count {its}")
            assert conv and abs(rep.iterations - its) <= 1, (name, kind, rep.iterations, its)
            assert np.array_equal(xm[fixed != 0], x[fixed != 0])
    g.close()


# ---- 4. tensor_ops and the facade ----------------------------------------------------------------------------------------
def test_constrained_solve_equals_the_capi_route():
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 96, 64, 3
    fixed = region(W, H, 3)
    gx, gy, f = field(W, H, Cn, 21, -8, 8), field(W, H, Cn, 22, -8, 8), field(W, H, Cn, 23, 0.0, 255.0)
    v = field(W, H, Cn, 24, 0.0, 255.0)
    lam = np.full((H, W), 0.0625, np.float32)
    t = [torch.from_numpy(a).to(DEV) for a in (gx, gy, f, v)]
    for kind in KINDS:
        g = capi.Grid(W, H, Cn, weighted=True)
        g.mg_set_hierarchy(kind)
        g.set_weights(None, None, lam, fixed=fixed)
        g.assemble_constrained_rhs(gx, gy, f, v, init_x=True)
        g.mg_conjugate_gradient(1e-10, 200)
        want = np.stack([g.get_x(c) for c in range(Cn)], axis=-1)
        want8 = g.store_u8()
        g.close()
        x = tensor_ops.constrained_solve(*t, torch.from_numpy(fixed).to(DEV) != 0, 200, data_weight=0.0625, out_dtype=torch.float64,
                                         hierarchy=kind)
        assert np.array_equal(x.cpu().numpy(), want), kind
        x8 = tensor_ops.constrained_solve(*t, torch.from_numpy(fixed).to(DEV), 200, data_weight=torch.from_numpy(lam).to(DEV),
                                          hierarchy=kind)
        assert x8.dtype == torch.uint8 and np.array_equal(x8.cpu().numpy(), want8), kind


def perez_direct(src, tgt, mask, mixed):
    """The Perez system on the region (4-neighbour Laplacian, neighbours outside the canvas absent) by scipy, per channel."""
    H, W, Cn = src.shape
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    gx, gy = np.zeros_like(s), np.zeros_like(s)
    gx[:, :-1] = s[:, 1:] - s[:, :-1]
    gy[:-1] = s[1:] - s[:-1]
    if mixed:
        tx, ty = t[:, 1:] - t[:, :-1], t[1:] - t[:-1]
        gx[:, :-1] = np.where(np.abs(tx) > np.abs(gx[:, :-1]), tx, gx[:, :-1])
        gy[:-1] = np.where(np.abs(ty) > np.abs(gy[:-1]), ty, gy[:-1])
    out = t.copy()
    for c in range(Cn):
        A_ff, b_f, free = ch.free_system(W, H, None, None, None, mask == 0, gx[..., c], gy[..., c], None, t[..., c])
        plane = t[..., c].copy()
        plane.ravel()[free] = sla.spsolve(A_ff.tocsc(), b_f)
        out[..., c] = plane
    return out


@pytest.mark.parametrize("mixed", [False, True])
def test_seamless_clone_constrained(mixed):
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 120, 90, 3
    g = rng(40)
    src = g.integers(60, 200, (H, W, Cn), dtype=np.uint8)
    tgt = (np.linspace(40, 210, W)[None, :, None] + g.uniform(-8, 8, (H, W, Cn))).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    interior = (((xx - 60) / 35.0) ** 2 + ((yy - 45) / 25.0) ** 2 < 1.0).astype(np.uint8)
    border = (((xx - 5) / 40.0) ** 2 + ((yy - 45) / 30.0) ** 2 < 1.0).astype(np.uint8)     # crosses x = 0
    ts, tt = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    for mask in (interior, border):
        got = tensor_ops.seamless_clone_constrained(ts, tt, torch.from_numpy(mask).to(DEV), 200, mixed=mixed).cpu().numpy()
        want = perez_direct(src, tgt, mask, mixed)
        assert np.array_equal(got[mask == 0], tgt[mask == 0])
        # the u8 result is the truncated clamp of a solution that is within 1e-6 max|x| of the direct one
        tol = 1e-6 * np.abs(want).max()
        lo, hi = np.clip(want - tol, 0, 255).astype(np.uint8), np.clip(want + tol, 0, 255).astype(np.uint8)
        assert np.all((got >= lo) & (got <= hi))
    with pytest.raises(capi.CcpError):
        tensor_ops.seamless_clone(ts, tt, torch.from_numpy(border).to(DEV), 10)
    tensor_ops.seamless_clone(ts, tt, torch.from_numpy(interior).to(DEV), 10)


def test_facade_solve_constrained(tmp_path):
    libdir = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib")
    exe = os.path.join(str(tmp_path), "constrained_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "constrained_driver.cpp"), "-L" + libdir, "-lccp_gs",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, Cn = 70, 45, 3
    fixed = region(W, H, 2)
    gx, gy, f = field(W, H, Cn, 31, -8, 8), field(W, H, Cn, 32, -8, 8), field(W, H, Cn, 33, 0.0, 255.0)
    v = field(W, H, Cn, 34, 0.0, 255.0)
    lam = np.full((H, W), 0.1, np.float32)
    arrays = [gx, gy, f, v, None, None, lam]
    fin, fout = os.path.join(str(tmp_path), "c.in"), os.path.join(str(tmp_path), "c.out")
    with open(fin, "wb") as fh:
        fh.write(np.array([W, H, Cn] + [a is not None for a in arrays], dtype="<i4").tobytes())
        for a in arrays:
            if a is not None:
                fh.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        fh.write(fixed.tobytes())
    for kind in KINDS:
        p = subprocess.run([exe, kind, "200", fin, fout], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        out = np.fromfile(fout, dtype=np.uint8).reshape(H, W, Cn)
        g = capi.Grid(W, H, Cn, weighted=True)
        g.mg_set_hierarchy(kind)
        g.set_weights(None, None, lam, fixed=fixed)
        g.assemble_constrained_rhs(gx, gy, f, v, init_x=True)
        g.mg_conjugate_gradient(1e-10, 200)
        assert np.array_equal(out, g.store_u8()), kind
        g.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def desc(ptr, dtype, sy, sx, sc):
    return capi.DeviceArray(ptr, dtype, 0, 0, sy, sx, sc)


def loaded_library(name):
    """The path of the shared library `name` as this process has it mapped: the HIP runtime the handles already use."""
    with open("/proc/self/maps") as fh:
        for line in fh:
            if name in line:
                return line.split()[-1]
    raise RuntimeError(f"{name} is not loaded")


def test_refusals():
    W, H, Cn = 24, 16, 1
    L = capi.load()
    by = C.byref
    f32 = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    u8 = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    fd, ud = desc(f32.data_ptr(), capi.DTYPE_F32, W, 1, 1), desc(u8.data_ptr(), capi.DTYPE_U8, W, 1, 1)
    n = C.c_int64()
    # structured and mask handles: UNSUPPORTED
    for other in (capi.Grid(W, H, Cn), capi.Grid(W, H, Cn, mask=np.ones((H, W), np.uint8))):
        h = other.h
        assert L.ccp_grid_set_weights_constrained_host(h, None, None, None, 0, None, 0) == UNSUPPORTED
        assert L.ccp_grid_set_weights_constrained_device(h, None, None, None, by(ud)) == UNSUPPORTED
        assert L.ccp_grid_assemble_constrained_rhs(h, None, None, 0, None, 0, None, 0, 0) == UNSUPPORTED
        assert L.ccp_grid_assemble_constrained_rhs_device(h, None, None, None, None, 0) == UNSUPPORTED
        assert L.ccp_grid_constraint_info(h, by(n), None, None) == UNSUPPORTED
        other.close()
    h = C.c_void_p()
    both = capi.GridDesc(8, 8, 1, 0, 8, 0, 0, capi.GRID_WEIGHTED | capi.GRID_DIRICHLET_MASK)
    assert L.ccp_grid_create(by(both), by(h)) == UNSUPPORTED and not h.value
    # before an operator exists: STATE
    g = capi.Grid(W, H, Cn, weighted=True)
    assert L.ccp_grid_assemble_constrained_rhs(g.h, None, None, 0, None, 0, None, 0, 0) == STATE
    assert L.ccp_grid_assemble_constrained_rhs_device(g.h, None, None, None, by(fd), 0) == STATE
    assert L.ccp_grid_constraint_info(g.h, by(n), None, None) == STATE
    # bad weights with a valid mask leave no operator
    fixed = random_fixed(W, H, 1)
    g.set_weights(fixed=fixed)
    assert g.constraint_info()[0] == int(fixed.sum())
    for bad in (-1.0, np.nan, np.inf):
        for which in range(3):
            arrs = [np.ones((H, W), np.float32) for _ in range(3)]
            ys, xs = np.nonzero(fixed) if which == 2 else np.nonzero(fixed == 0)      # a fixed pixel's weights are checked too
            arrs[which][ys[0], min(xs[0], W - 2)] = bad
            with pytest.raises(capi.CcpError) as e:
                g.set_weights(*arrs, fixed=fixed)
            assert e.value.status == BAD_ARG
            assert L.ccp_grid_mg_apply(g.h, 2) == STATE
            assert L.ccp_grid_assemble_constrained_rhs(g.h, None, None, 0, None, 0, None, 0, 0) == STATE
    g.set_weights(fixed=fixed)
    # short strides of the host twins
    z = np.zeros((H, W), np.float32)
    assert L.ccp_grid_set_weights_constrained_host(g.h, z.ctypes.data, None, None, 4 * W - 1, fixed.ctypes.data, W) == BAD_ARG
    assert L.ccp_grid_set_weights_constrained_host(g.h, None, None, None, 0, fixed.ctypes.data, W - 1) == BAD_ARG
    g.set_weights(fixed=fixed)
    assert L.ccp_grid_assemble_constrained_rhs(g.h, None, None, 0, None, 0, z.ctypes.data, 4 * W - 1, 0) == BAD_ARG
    # the device twins: host pointers, pinned memory, a null pointer, a wrong dtype, a negative stride
    host = np.zeros((H, W), np.uint8)
    pinned = torch.zeros((H, W), dtype=torch.uint8).pin_memory()
    bads = [desc(host.ctypes.data, capi.DTYPE_U8, W, 1, 1), desc(pinned.data_ptr(), capi.DTYPE_U8, W, 1, 1), desc(0, capi.DTYPE_U8, W, 1, 1),
            desc(u8.data_ptr(), 7, W, 1, 1), desc(u8.data_ptr(), capi.DTYPE_U8, -W, 1, 1)]
    for k, bad in enumerate(bads):
        assert L.ccp_grid_set_weights_constrained_device(g.h, None, None, None, by(bad)) == BAD_ARG, k
        assert L.ccp_grid_assemble_constrained_rhs_device(g.h, None, None, None, by(bad), 0) == BAD_ARG, k
        assert g.constraint_info()[0] == int(fixed.sum())              # refused before anything changed
    assert L.ccp_grid_assemble_constrained_rhs_device(g.h, by(ud), None, None, None, 0) == BAD_ARG        # gx must be F32
    # managed memory
    hip = C.CDLL(loaded_library("libamdhip64"))
    hip.hipMallocManaged.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    if hip.hipMallocManaged(by(p), W * H, 1) == 0:
        m = desc(p.value, capi.DTYPE_U8, W, 1, 1)
        assert L.ccp_grid_set_weights_constrained_device(g.h, None, None, None, by(m)) == BAD_ARG
        assert L.ccp_grid_assemble_constrained_rhs_device(g.h, None, None, None, by(m), 0) == BAD_ARG
        hip.hipFree(p)
    # inputs may overlap (broadcast): accepted; Python refuses a CPU tensor before the library
    assert L.ccp_grid_set_weights_constrained_device(g.h, None, None, None, by(desc(u8.data_ptr(), capi.DTYPE_U8, 0, 0, 0))) == 0
    with pytest.raises(ValueError):
        g.set_weights_tensor(fixed=torch.zeros((H, W), dtype=torch.uint8))
    with pytest.raises(ValueError):
        g.assemble_constrained_rhs_tensor(values=torch.zeros((H, W, Cn), dtype=torch.int32, device=DEV))
    g.close()
