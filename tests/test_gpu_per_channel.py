"""GPU: one operator per channel on a weighted grid handle (include/ccp_gs.h, ccp_grid_set_weights_per_channel_device).

In every test the reference is a ONE-CHANNEL weighted handle given channel c's slices through the existing setters
(set_weights_tensor), and equality is of bits: the raw float64 of every plane, of b and x, `iterations` and `converged`,
`last_l1_step` as bits.  The numpy models of the shared operator's tests (tests/per_channel_helpers.py) are a second
reference for the operator and the right-hand side.  Shapes (W x H x C): 131x67x3 (three tiles each way, odd sides, two
levels above the tail), 70x37x5 (five channels: two of the batched kernels' channel groups on a shared operator; fixed
pixels and dead pixels), 40x24x2 (one tile), 5x3x2 (the tail alone)."""
import numpy as np
import pytest
import torch

import constrained_helpers as ch
import mixed_helpers as mh
import per_channel_helpers as pch
from coursecomputationalphotography_amd import capi, tensor_ops

pytestmark = pytest.mark.gpu

BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
DEV = torch.device("cuda", 0)
MODES = [("galerkin", "f64", "point"), ("rescaled", "f64", "point"), ("rescaled", "f32", "point"), ("rescaled", "f64", "line")]
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, what):
    assert np.array_equal(bits(a), bits(b)), (what, float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)))))


def same_report(a, b, what):
    assert a.iterations == b.iterations and a.converged == b.converged, (what, a.iterations, b.iterations, a.converged, b.converged)
    assert bits(a.last_l1_step) == bits(b.last_l1_step), (what, a.last_l1_step, b.last_l1_step)


def system(W, H, C):
    """(numpy operators, numpy inputs, the same as device tensors): made once per shape."""
    if (W, H, C) not in _cache:
        ops, ins = pch.operators(W, H, C), pch.inputs(W, H, C)
        _cache[(W, H, C)] = (ops, ins, [torch.from_numpy(a).to(DEV) for a in ops], [torch.from_numpy(a).to(DEV) for a in ins])
    return _cache[(W, H, C)]


def configure(g, kind="rescaled", precision="f64", smoother="point", channels="sequential"):
    g.mg_set_hierarchy(kind)
    g.mg_set_precision(precision)
    g.mg_set_smoother(smoother)
    g.mg_set_channels(channels)
    return g


def stacked(W, H, C, with_fixed=True, **mode):
    """The handle under test: C channels, one operator each."""
    _, _, (wx, wy, lam, fixed), _ = system(W, H, C)
    g = configure(capi.Grid(W, H, C, weighted=True), **mode)
    g.set_weights_per_channel_tensor(wx, wy, lam, fixed if with_fixed else None)
    assert g.operator_channels() == C
    return g


def single(W, H, C, c, with_fixed=True, **mode):
    """The reference: a one-channel handle given channel c's slices through the existing setter."""
    ops, _, (wx, wy, lam, fixed), _ = system(W, H, C)
    g = configure(capi.Grid(W, H, 1, weighted=True), **mode)
    fx = fixed[..., c] if with_fixed and pch.channel_fixed(ops[3], c) is not None else None
    g.set_weights_tensor(wx[..., c], wy[..., c], lam[..., c], fixed=fx)
    assert g.operator_channels() == 1
    return g


def assemble(g, tins, c=None, init=True):
    gx, gy, f, values = tins if c is None else [t[..., c:c + 1] for t in tins]
    g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=init)


# ---- 1. the operator and the hierarchy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("kind", ["galerkin", "rescaled"])
@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_every_level_of_every_channel_is_the_one_channel_handles(W, H, C, kind, with_fixed):
    ops = system(W, H, C)[0]
    g = stacked(W, H, C, with_fixed, kind=kind)
    for c in range(C):
        r = single(W, H, C, c, with_fixed, kind=kind)
        want, got = r.mg_levels(), g.mg_levels(channel=c)
        assert len(want) == len(got)
        for k, (a, b) in enumerate(zip(got, want)):
            for name, p, q in zip(("d", "we", "ws"), a, b):
                same(p, q, f"{W}x{H} {kind} channel {c} level {k} {name}")
            for name, p, q in zip(("d", "we", "ws"), g.mg_level(k, channel=c), b):
                same(p, q, f"mg_level {k} channel {c} {name}")
        assert g.constraint_info(channel=c) == r.constraint_info(), c
        # the numpy model: level 0 and the counts
        fx = pch.channel_fixed(ops[3], c) if with_fixed else None
        lv = ch.hierarchy(W, H, ops[0][..., c], ops[1][..., c], ops[2][..., c], fx, kind)
        same(got[0][0], lv[0].d, f"model d channel {c}")
        same(got[0][1], lv[0].we, f"model we channel {c}")
        assert g.constraint_info(channel=c) == ch.counts(lv[0]), c
        r.close()
    assert g.constraint_info() == g.constraint_info(channel=0)
    same(g.mg_levels()[0][0], g.mg_levels(channel=0)[0][0], "mg_level reports channel 0")
    g.close()


# ---- 2. the right-hand side ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_b_and_x_of_every_channel(W, H, C, init):
    ops, ins, _, tins = system(W, H, C)
    g = stacked(W, H, C)
    g.fill_x(3.0)
    assemble(g, tins, init=init)
    for c in range(C):
        r = single(W, H, C, c)
        r.fill_x(3.0)
        assemble(r, tins, c, init=init)
        same(g.get_b(c), r.get_b(0), f"b channel {c}")
        same(g.get_x(c), r.get_x(0), f"x channel {c}")
        lv = pch.channel_levels(ops, c)
        same(g.get_b(c), pch.channel_rhs(lv, ins, c), f"model b channel {c}")
        r.close()
    g.close()


def test_the_host_twin_assembles_the_same():
    W, H, C = 70, 37, 5
    _, ins, _, tins = system(W, H, C)
    g, h = stacked(W, H, C), stacked(W, H, C)
    assemble(g, tins)
    h.assemble_constrained_rhs(*ins, init_x=True)
    for c in range(C):
        same(h.get_b(c), g.get_b(c), f"b channel {c}")
        same(h.get_x(c), g.get_x(c), f"x channel {c}")
    g.close()
    h.close()


# ---- 3. sequential solves -----------------------------------------------------------------------------------------------------
def solve_all(g, tins, eps, cap, nu):
    assemble(g, tins)
    reps = g.mg_conjugate_gradient(eps, cap, nu)
    return reps, [g.get_x(c) for c in range(g.C)]


@pytest.mark.parametrize("kind,precision,smoother", MODES)
@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_sequential_solve_is_the_one_channel_solve(W, H, C, kind, precision, smoother):
    _, _, _, tins = system(W, H, C)
    mode = dict(kind=kind, precision=precision, smoother=smoother)
    nu = 1 if smoother == "line" else 2
    g = stacked(W, H, C, **mode)
    assemble(g, tins)
    eps = 1e-10 * float(np.linalg.norm(g.get_b(0)))
    reps, xs = solve_all(g, tins, eps, 200, nu)
    print(f"{W}x{H}x{C} {kind} {precision} {smoother}: iterations {[r.iterations for r in reps]} converged {[r.converged for r in reps]}")
    rr, bb = g.residual_norm2()
    assemble(g, tins)
    g.mg_apply(nu)
    zs = [g.get_x(c) for c in range(C)]
    g.b_from_x()
    for c in range(C):
        r = single(W, H, C, c, **mode)
        want, xr = solve_all(r, [t[..., c:c + 1] for t in tins], eps, 200, nu)
        same(xs[c], xr[0], f"x channel {c}")
        same_report(reps[c], want[0], f"report channel {c}")
        r1, b1 = r.residual_norm2()
        assert bits(rr[c]) == bits(r1[0]) and bits(bb[c]) == bits(b1[0]), (c, rr[c], r1[0])
        assemble(r, tins, c)
        r.mg_apply(nu)
        same(zs[c], r.get_x(0), f"mg_apply channel {c}")
        r.b_from_x()
        same(g.get_b(c), r.get_b(0), f"b_from_x channel {c}")
        r.close()
    g.close()


# ---- 4. the batched solve (k_pco_tile, k_pco_restrict, k_pco_tail, k_pco_apply) ------------------------------------------------
@pytest.mark.parametrize("kind", ["galerkin", "rescaled"])
@pytest.mark.parametrize("W,H,C", pch.SHAPES)
def test_batched_is_sequential_bit_for_bit(W, H, C, kind):
    _, _, _, tins = system(W, H, C)
    g = stacked(W, H, C, kind=kind)
    assemble(g, tins)
    eps = 1e-10 * float(np.linalg.norm(g.get_b(0)))
    want, xw = solve_all(g, tins, eps, 200, 2)
    assemble(g, tins)
    g.mg_apply(2)
    zw = [g.get_x(c) for c in range(C)]
    g.mg_set_channels("batched")
    got, xg = solve_all(g, tins, eps, 200, 2)
    its = [r.iterations for r in want]
    print(f"{W}x{H}x{C} {kind}: iterations {its}")
    for c in range(C):
        same(xg[c], xw[c], f"x channel {c}")
        same_report(got[c], want[c], f"report channel {c}")
    assemble(g, tins)
    g.mg_apply(2)
    for c in range(C):
        same(g.get_x(c), zw[c], f"mg_apply channel {c}")
    assert all(r.converged for r in want), its
    if kind == "rescaled":
        # the counts the numpy model establishes on the CPU for this very call (tests/test_per_channel_helpers.py): the
        # channels stop at different iterations, sequential and batched alike.  (On the Galerkin hierarchy the model and
        # the device differ by one iteration in one channel, 22 against 21 at 131x67, so only batched == sequential is
        # asserted there.)
        assert its == pch.HANDLE_COUNTS[(W, H, C)], its
        assert [r.iterations for r in got] == pch.HANDLE_COUNTS[(W, H, C)]
    g.close()


@pytest.mark.parametrize("cap", [0, 10, 17])
def test_batched_with_a_cap_that_leaves_a_channel_unconverged(cap):
    W, H, C = 131, 67, 3
    _, _, _, tins = system(W, H, C)
    g = stacked(W, H, C)
    assemble(g, tins)
    eps = 1e-10 * float(np.linalg.norm(g.get_b(0)))
    want, xw = solve_all(g, tins, eps, cap, 2)
    g.mg_set_channels("batched")
    got, xg = solve_all(g, tins, eps, cap, 2)
    for c in range(C):
        same(xg[c], xw[c], f"x channel {c}")
        same_report(got[c], want[c], f"report channel {c}")
    assert not want[1].converged and want[1].iterations == cap
    if cap >= 10:
        assert want[0].converged and want[0].iterations < cap
    g.close()


@pytest.mark.parametrize("nu", [1, 4])
def test_batched_other_sweep_counts(nu):
    W, H, C = 70, 37, 5
    _, _, _, tins = system(W, H, C)
    g = stacked(W, H, C)
    assemble(g, tins)
    eps = 1e-10 * float(np.linalg.norm(g.get_b(0)))
    want, xw = solve_all(g, tins, eps, 30, nu)
    g.mg_set_channels("batched")
    got, xg = solve_all(g, tins, eps, 30, nu)
    for c in range(C):
        same(xg[c], xw[c], f"x channel {c}")
        same_report(got[c], want[c], f"report channel {c}")
    g.close()


# ---- 5. broadcast views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,C", [(70, 37, 5), (5, 3, 2)])
def test_broadcast_views_give_the_shared_operator(W, H, C):
    _, _, (wx, wy, lam, fixed), tins = system(W, H, C)
    c = 3 if C == 5 else 1
    planes = (wx[..., c], wy[..., c], lam[..., c])
    fx = fixed[..., c] if C == 5 else None
    shared = configure(capi.Grid(W, H, C, weighted=True))
    shared.set_weights_tensor(*planes, fixed=fx)
    g = configure(capi.Grid(W, H, C, weighted=True))
    g.set_weights_per_channel_tensor(*planes, fx)                    # H x W tensors: stride_c = 0
    g2 = configure(capi.Grid(W, H, C, weighted=True))
    g2.set_weights_per_channel_tensor(*[p.unsqueeze(-1).expand(H, W, C) for p in planes],   # H x W x C views whose stride_c is 0
                                      None if fx is None else fx.unsqueeze(-1).expand(H, W, C))
    assemble(shared, tins)
    eps = 1e-10 * float(np.linalg.norm(shared.get_b(0)))
    for channels in ("sequential", "batched"):
        shared.mg_set_channels(channels)
        want, xw = solve_all(shared, tins, eps, 200, 2)
        for h in (g, g2):
            h.mg_set_channels(channels)
            got, xg = solve_all(h, tins, eps, 200, 2)
            for k in range(C):
                same(xg[k], xw[k], f"{channels} x channel {k}")
                same_report(got[k], want[k], f"{channels} report channel {k}")
    if C == 2:                                                       # wy = 1 everywhere is wy = None
        g2.set_weights_per_channel_tensor(planes[0], None, planes[2], None)
        g.set_weights_per_channel_tensor(planes[0], torch.tensor(1.0, device=DEV).expand(H, W, C), planes[2], None)
        for k in range(C):
            same(g2.mg_levels(channel=k)[0][0], g.mg_levels(channel=k)[0][0], "default wy")
    for h in (shared, g, g2):
        h.close()


# ---- 6. switching ---------------------------------------------------------------------------------------------------------------
def test_switching_between_the_shared_and_the_per_channel_operator():
    W, H, C = 70, 37, 5
    _, _, (wx, wy, lam, fixed), tins = system(W, H, C)
    fresh_pc = stacked(W, H, C)
    assemble(fresh_pc, tins)
    eps = 1e-10 * float(np.linalg.norm(fresh_pc.get_b(0)))
    want_pc, x_pc = solve_all(fresh_pc, tins, eps, 200, 2)
    fresh_sh = configure(capi.Grid(W, H, C, weighted=True))
    fresh_sh.set_weights_tensor(wx[..., 3], wy[..., 3], lam[..., 3], fixed=fixed[..., 3])
    want_sh, x_sh = solve_all(fresh_sh, tins, eps, 200, 2)

    def is_pc(g, what, channels="sequential"):
        assert g.operator_channels() == C
        g.mg_set_channels(channels)
        got, xs = solve_all(g, tins, eps, 200, 2)
        for c in range(C):
            same(xs[c], x_pc[c], f"{what}: x channel {c}")
            same_report(got[c], want_pc[c], f"{what}: report channel {c}")

    def is_shared(g, what):
        assert g.operator_channels() == 1
        g.mg_set_channels("sequential")
        got, xs = solve_all(g, tins, eps, 200, 2)
        for c in range(C):
            same(xs[c], x_sh[c], f"{what}: x channel {c}")
            same_report(got[c], want_sh[c], f"{what}: report channel {c}")

    # per-channel -> shared -> per-channel
    g = stacked(W, H, C)
    is_pc(g, "first")
    g.set_weights_tensor(wx[..., 3], wy[..., 3], lam[..., 3], fixed=fixed[..., 3])
    is_shared(g, "back to shared")
    g.set_weights_per_channel_tensor(wx, wy, lam, fixed)
    is_pc(g, "per-channel again")
    # a mode change in between: batched, the other hierarchy and back, f32 and back
    is_pc(g, "batched", "batched")
    g.mg_set_hierarchy("galerkin")
    g.mg_set_hierarchy("rescaled")
    g.mg_set_precision("f32")
    g.mg_set_channels("sequential")
    g.mg_conjugate_gradient(eps, 3, 2)
    g.mg_set_precision("f64")
    is_pc(g, "after the mode walk", "batched")
    is_pc(g, "after the mode walk, sequential")
    g.close()
    # shared -> per-channel
    g = configure(capi.Grid(W, H, C, weighted=True))
    g.set_weights_tensor(wx[..., 3], wy[..., 3], lam[..., 3], fixed=fixed[..., 3])
    is_shared(g, "shared first")
    g.set_weights_per_channel_tensor(wx, wy, lam, fixed)
    is_pc(g, "shared -> per-channel")
    g.close()
    fresh_pc.close()
    fresh_sh.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])               # k_weighted_coef's verdict and k_weighted_coef_fixed's
@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf")])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_bad_weight_in_one_channel_only(which, bad, with_mask):
    W, H, C = 40, 24, 2
    _, _, (wx, wy, lam, fixed), tins = system(W, H, C)
    fixed = fixed if with_mask else None
    planes = [wx.clone(), wy.clone(), lam.clone()]
    planes[which][5, 7, 1] = bad
    g = stacked(W, H, C, with_mask)
    with pytest.raises(capi.CcpError) as e:
        g.set_weights_per_channel_tensor(*planes, fixed)
    assert e.value.status == BAD_ARG
    for call in (lambda: g.mg_conjugate_gradient(1e-6, 5, 2), lambda: g.operator_channels(), lambda: assemble(g, tins),
                 lambda: g.constraint_info(channel=1)):
        with pytest.raises(capi.CcpError) as e:
            call()
        assert e.value.status == STATE
    g.set_weights_per_channel_tensor(wx, wy, lam, fixed)             # a valid set brings the handle back
    assert g.operator_channels() == C
    g.close()


def test_other_handles_and_short_views_are_refused():
    W, H, C = 40, 24, 2
    _, _, (wx, wy, lam, fixed), _ = system(W, H, C)
    for g in (capi.Grid(W, H, C), capi.Grid(W, H, C, mask=mh.disc_and_blob(W, H))):
        with pytest.raises(capi.CcpError) as e:
            g.set_weights_per_channel_tensor(wx, wy, lam, None)
        assert e.value.status == UNSUPPORTED
        n = capi.C.c_int32(7)
        assert g.L.ccp_grid_operator_channels(g.h, capi.C.byref(n)) == UNSUPPORTED and n.value == 7
        g.close()
    g = stacked(W, H, C)
    before = g.mg_levels(channel=1)[0][0]
    # a view whose channel 1 lies beyond its allocation: refused before anything is enqueued
    short = torch.ones(H, W, dtype=torch.float64, device=DEV)
    arr = capi.DeviceArray(short.data_ptr(), capi.DTYPE_F64, 0, 0, W, 1, 1 << 40)
    assert g.L.ccp_grid_set_weights_per_channel_device(g.h, capi.C.byref(arr), None, None, None) == BAD_ARG
    u8 = capi.DeviceArray(short.data_ptr(), capi.DTYPE_U8, 0, 0, W, 1, 0)
    assert g.L.ccp_grid_set_weights_per_channel_device(g.h, capi.C.byref(u8), None, None, None) == BAD_ARG   # weights are F32 / F64
    assert g.operator_channels() == C                                # the installed operator is still there
    same(g.mg_levels(channel=1)[0][0], before, "untouched")
    for bad in (-1, C):
        assert g.L.ccp_grid_mg_level_channel(g.h, bad, 0, None, None, None, None, None, None) == BAD_ARG
        assert g.L.ccp_grid_constraint_info_channel(g.h, bad, None, None, None) == BAD_ARG
    g.close()


@pytest.mark.parametrize("precision,smoother", [("f32", "point"), ("f64", "line")])
def test_batched_with_f32_or_line_stays_unsupported(precision, smoother):
    W, H, C = 40, 24, 2
    _, _, _, tins = system(W, H, C)
    g = stacked(W, H, C, precision=precision, smoother=smoother, channels="batched")
    assemble(g, tins)
    b0, x0 = [g.get_b(c) for c in range(C)], [g.get_x(c) for c in range(C)]
    for call in (lambda: g.mg_conjugate_gradient(1e-6, 5, 1), lambda: g.mg_apply(1)):
        with pytest.raises(capi.CcpError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    for c in range(C):
        same(g.get_b(c), b0[c], "b untouched")
        same(g.get_x(c), x0[c], "x untouched")
    g.close()


# ---- 9. tensor_ops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", ["sequential", "batched"])
def test_weighted_and_constrained_solve_with_stacked_weights(channels):
    W, H, C = 70, 37, 5
    _, _, (wx, wy, lam, fixed), (gx, gy, f, values) = system(W, H, C)
    for out_dtype in (torch.uint8, torch.float64):
        got = tensor_ops.weighted_solve(gx, gy, f, 200, wx=wx, wy=wy, data_weight=lam, out_dtype=out_dtype, hierarchy="rescaled",
                                        channels=channels)
        con = tensor_ops.constrained_solve(gx, gy, f, values, fixed, 200, wx=wx, wy=wy, data_weight=lam, out_dtype=out_dtype,
                                           channels=channels)
        assert got.shape == con.shape == (H, W, C) and got.dtype == out_dtype
        for c in range(C):
            one = tensor_ops.weighted_solve(gx[..., c:c + 1], gy[..., c:c + 1], f[..., c:c + 1], 200, wx=wx[..., c], wy=wy[..., c],
                                            data_weight=lam[..., c], out_dtype=out_dtype, hierarchy="rescaled")
            assert torch.equal(got[..., c:c + 1], one), c
            two = tensor_ops.constrained_solve(gx[..., c:c + 1], gy[..., c:c + 1], f[..., c:c + 1], values[..., c:c + 1], fixed[..., c], 200,
                                               wx=wx[..., c], wy=wy[..., c], data_weight=lam[..., c], out_dtype=out_dtype)
            assert torch.equal(con[..., c:c + 1], two), c
    # a mixed call: 3-D wx beside 2-D wy and a scalar data weight
    mixed = tensor_ops.weighted_solve(gx, gy, f, 200, wx=wx, wy=wy[..., 1], data_weight=0.5, out_dtype=torch.float64, hierarchy="rescaled",
                                      channels=channels)
    one = tensor_ops.weighted_solve(gx[..., 2:3], gy[..., 2:3], f[..., 2:3], 200, wx=wx[..., 2], wy=wy[..., 1], data_weight=0.5,
                                    out_dtype=torch.float64, hierarchy="rescaled")
    assert torch.equal(mixed[..., 2:3], one)


def test_two_dimensional_weights_take_todays_path():
    W, H, C = 40, 24, 2
    _, _, (wx, wy, lam, fixed), (gx, gy, f, values) = system(W, H, C)
    got = tensor_ops.weighted_solve(gx, gy, f, 100, wx=wx[..., 1], wy=wy[..., 1], data_weight=lam[..., 1], out_dtype=torch.float64,
                                    hierarchy="rescaled")
    g = configure(capi.Grid(W, H, C, weighted=True))
    g.set_weights_tensor(wx[..., 1], wy[..., 1], lam[..., 1])
    assert g.operator_channels() == 1
    g.assemble_weighted_rhs_tensor(gx, gy, f, init_x=True)
    g.mg_conjugate_gradient(1e-10, 100, 2)
    assert torch.equal(got, g.get_x_tensor())
    g.close()
