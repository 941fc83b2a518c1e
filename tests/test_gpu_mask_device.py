"""GPU: ccp_grid_set_mask_device (capi.Grid.set_mask_tensor) against ccp_grid_set_mask_host on the same mask: two handles,
one set each way, must agree bit for bit on everything the mask decides -- x and b outside the region, the region
assembly (which reads mask_edge), red-black sweeps (the tile census), a multigrid PCG solve (the hierarchy), the u8
composite -- and on the border verdict (assemble_clone's refusal).  Any dtype and strides of the mask view, a second mask
on one handle, the refusals, row blocks given the whole-canvas tensor, and tensor_ops with a CUDA mask."""
import ctypes as C

import numpy as np
import pytest

from coursecomputationalphotography_amd import lab8_workload as L8

pytestmark = pytest.mark.gpu
BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
SHAPES = [(33, 9), (130, 67), (1031, 40)]
KINDS = ["disc", "lab8", "random", "zero", "border"]


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def make_mask(kind, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "disc":
        r = 0.35 * min(W, H)                                   # clear of the border at every shape
        return (((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < r * r).astype(np.uint8)
    if kind == "lab8":                                             # (empty at 33 x 9: the generator's quads have no room there)
        return (L8.merge(L8.inputs(W, H))["mask"] != 0).astype(np.uint8)
    if kind == "random":
        return (rng(W * H).random((H, W)) < 0.5).astype(np.uint8)
    if kind == "zero":
        return np.zeros((H, W), np.uint8)
    m = make_mask("disc", W, H)                                    # "border": the disc and pixels on three outer lines
    m[0, W // 3] = m[H // 2, W - 1] = m[H - 1, 1] = 1
    return m


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def fields(W, H, Cn, seed):
    r = rng(seed)
    return (r.uniform(-255, 255, (H, W, Cn)).astype(np.float32), r.uniform(-255, 255, (H, W, Cn)).astype(np.float32),
            r.integers(0, 256, (H, W, Cn), dtype=np.uint8), r.uniform(-1, 1, (H, W, Cn)))


def planes(g, which="x"):
    get = g.get_x if which == "x" else g.get_b
    return np.stack([get(ch) for ch in range(g.C)], axis=-1)


def attempt(fn):
    """fn()'s result, or the status it was refused with: two handles in one state give the same either way."""
    from coursecomputationalphotography_amd import capi
    try:
        return fn()
    except capi.CcpError as e:
        return ("status", e.status)


def handle_state(g, W, H, Cn, seed=5):
    """Everything the mask decides on handle `g`, as a list of (name, array or refusal)."""
    gx, gy, canvas, x0 = fields(W, H, Cn, seed)
    out = []
    for ch in range(Cn):
        g.set_x(x0[..., ch], ch)
    out.append(("x after set_x", planes(g)))
    g.assemble_region_rhs(gx, gy, canvas, init_x=True)
    out.append(("b", planes(g, "b")))
    out.append(("x init", planes(g)))
    out.append(("sweeps", attempt(lambda: (g.sweep(16), planes(g))[1])))
    g.assemble_region_rhs(gx, gy, canvas, init_x=True)

    def solve():
        reps = g.mg_conjugate_gradient(1e-10, 60, 2)
        return np.concatenate([planes(g).ravel(), [r.iterations for r in reps], [r.converged for r in reps]])
    out.append(("mg pcg", attempt(solve)))
    out.append(("composite", g.store_u8_composite(canvas)))
    out.append(("clone", attempt(lambda: (g.assemble_clone(canvas, canvas), planes(g, "b"))[1])))
    return out


def same_state(a, b):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, u), (_, v) in zip(a, b):
        if isinstance(u, tuple) or isinstance(v, tuple):
            assert u == v, name
        else:
            assert np.array_equal(u, v), name


_host_states = {}


def host_state(kind, W, H, Cn=3):
    """The reference side, computed once per mask and left unchanged."""
    from coursecomputationalphotography_amd import capi
    key = (kind, W, H, Cn)
    if key not in _host_states:
        g = capi.Grid(W, H, Cn, mask=make_mask(kind, W, H))
        _host_states[key] = handle_state(g, W, H, Cn)
        g.close()
    return _host_states[key]


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_device_mask_leaves_the_handle_as_the_host_mask(torch, kind, W, H):
    from coursecomputationalphotography_amd import capi
    mask = make_mask(kind, W, H)
    want = host_state(kind, W, H)
    g = capi.Grid(W, H, 3, mask=torch.from_numpy(mask).cuda())
    got = handle_state(g, W, H, 3)
    g.close()
    same_state(got, want)
    x_set = dict(got)["x after set_x"]
    assert not x_set[mask == 0].any() and (mask == 0).any()                # zero outside the region
    if mask.any():
        assert np.array_equal(x_set[mask != 0], fields(W, H, 3, 5)[3][mask != 0])
    clone = dict(got)["clone"]
    if kind == "border":
        assert clone == ("status", UNSUPPORTED) and dict(want)["clone"] == ("status", UNSUPPORTED)
    elif kind in ("disc", "lab8", "zero"):
        assert not isinstance(clone, tuple)                                 # clear of the border: served


@pytest.mark.parametrize("view", ["u8", "bool", "f32", "f64", "column_major", "window", "zero_stride"])
def test_any_dtype_and_strides_give_the_same_state(torch, view):
    from coursecomputationalphotography_amd import capi
    W, H = 130, 67
    mask = make_mask("lab8", W, H)
    t = torch.from_numpy(mask).cuda()
    if view == "bool":
        t = t != 0
    elif view == "f32":
        t = t.to(torch.float32) * 0.25                                       # non-zero means inside, whatever the value
    elif view == "f64":
        t = t.to(torch.float64) * -3.0
    elif view == "column_major":
        t = t.t().contiguous().t()
        assert t.stride() == (1, H)
    elif view == "window":
        big = torch.full((H + 7, W + 9), 255, dtype=torch.uint8, device="cuda")
        big[3:3 + H, 5:5 + W] = t
        t = big[3:3 + H, 5:5 + W]
    elif view == "zero_stride":                                               # one row broadcast down the canvas
        mask = np.broadcast_to(mask[H // 2], (H, W)).copy()
        t = torch.from_numpy(mask[0]).cuda().unsqueeze(0).expand(H, W)
        assert t.stride(0) == 0
    g = capi.Grid(W, H, 3, mask=np.ones((H, W), np.uint8))
    g.set_mask_tensor(t)
    got = handle_state(g, W, H, 3)
    g.close()
    if view == "zero_stride":
        gh = capi.Grid(W, H, 3, mask=mask)
        want = handle_state(gh, W, H, 3)
        gh.close()
    else:
        want = host_state("lab8", W, H)
    same_state(got, want)


def test_a_second_mask_on_one_handle_equals_a_fresh_handle(torch):
    """The tile census and the multigrid hierarchy of the first mask must be gone: sweeps and a PCG solve ran on it."""
    from coursecomputationalphotography_amd import capi
    W, H = 130, 67
    g = capi.Grid(W, H, 3, mask=torch.from_numpy(make_mask("random", W, H)).cuda())
    handle_state(g, W, H, 3)
    g.set_mask_tensor(torch.from_numpy(make_mask("disc", W, H)).cuda())
    got = handle_state(g, W, H, 3)
    g.close()
    same_state(got, host_state("disc", W, H))


def test_refusals_leave_x_and_b_untouched(torch):
    from coursecomputationalphotography_amd import capi
    W, H = 33, 9
    L = capi.load()
    good = torch.ones((H, W), dtype=torch.uint8, device="cuda")

    def arr(t, **over):
        sy, sx = t.stride()
        a = capi.DeviceArray(t.data_ptr(), capi.DTYPE_U8, 0, 0, sy, sx, 0)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    x0 = rng(3).uniform(-1, 1, (H, W))
    mask = make_mask("disc", W, H)
    g = capi.Grid(W, H, 1, mask=mask)
    g.set_x(x0)
    g.set_b(x0 * 2)
    before = g.get_x(), g.get_b()
    host_buf = np.ones((H, W), np.uint8)
    bad = [None,
           C.byref(arr(good, data=None)),
           C.byref(arr(good, data=host_buf.ctypes.data)),                    # not device memory
           C.byref(arr(good, stride_y=1 << 40)),                             # reaches beyond the allocation
           C.byref(arr(good, stride_x=-1)),
           C.byref(arr(good, dtype=7)),
           C.byref(arr(good, reserved=1))]
    for b in bad:
        assert L.ccp_grid_set_mask_device(g.h, b) == BAD_ARG
    assert L.ccp_grid_set_mask_device(None, C.byref(arr(good))) == BAD_ARG
    assert np.array_equal(g.get_x(), before[0]) and np.array_equal(g.get_b(), before[1])
    # ... and the region is still the disc
    g.fill_x(1.0)
    assert np.array_equal(g.get_x(), mask.astype(np.float64))
    with pytest.raises(ValueError):
        g.set_mask_tensor(good[:, :-1])
    with pytest.raises(ValueError):
        g.set_mask_tensor(good.cpu())
    g.close()

    plain = capi.Grid(W, H, 1)
    plain.set_x(x0)
    assert L.ccp_grid_set_mask_device(plain.h, C.byref(arr(good))) == STATE
    assert np.array_equal(plain.get_x(), x0)
    plain.close()

    weighted = capi.Grid(W, H, 1, weighted=True)
    assert L.ccp_grid_set_mask_device(weighted.h, C.byref(arr(good))) == UNSUPPORTED
    weighted.close()


@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("kind", ["lab8", "random", "border"])
def test_row_blocks_take_the_whole_canvas_tensor(torch, blocks, kind):
    """One card, no communicator: every block of a 130 x 67 canvas with ghost 2 reads its rows (and one either side) of
    the whole-canvas tensor; its b after the region assembly is that of the same block set by set_mask_host."""
    from coursecomputationalphotography_amd import capi
    W, H, Cn, ghost = 130, 67, 3, 2
    mask = make_mask(kind, W, H)
    gx, gy, canvas, _ = fields(W, H, Cn, 9)
    t = torch.from_numpy(mask).cuda()
    tgx, tgy, tcan = (torch.from_numpy(a).cuda() for a in (gx, gy, canvas))
    cuts = [H * k // blocks for k in range(blocks + 1)]
    for k in range(blocks):
        dev_g = capi.Grid(W, H, Cn, row_begin=cuts[k], row_count=cuts[k + 1] - cuts[k], ghost=ghost, mask=t)
        host_g = capi.Grid(W, H, Cn, row_begin=cuts[k], row_count=cuts[k + 1] - cuts[k], ghost=ghost, mask=mask)
        dev_g.assemble_region_rhs_tensor(tgx, tgy, tcan, init_x=True)
        host_g.assemble_region_rhs_tensor(tgx, tgy, tcan, init_x=True)
        torch.cuda.synchronize()
        assert np.array_equal(planes(dev_g, "b"), planes(host_g, "b")), k
        assert np.array_equal(planes(dev_g), planes(host_g)), k
        if kind == "border":
            for g in (dev_g, host_g):
                assert attempt(lambda: g.assemble_clone_tensor(tcan, tcan)) == ("status", UNSUPPORTED)
        dev_g.close()
        host_g.close()


@pytest.mark.parametrize("solver", ["GaussSeidel", "MultigridConjugateGradient"])
def test_tensor_ops_with_a_cuda_mask_return_the_same_tensors(torch, solver):
    from coursecomputationalphotography_amd import tensor_ops
    W, H, Cn = 130, 67, 3
    mask = make_mask("lab8", W, H)
    gx, gy, canvas, _ = fields(W, H, Cn, 21)
    source = rng(22).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    tgx, tgy, tcan, tsrc = (torch.from_numpy(a).cuda() for a in (gx, gy, canvas, source))
    for m in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask).cuda() != 0, torch.from_numpy(mask.astype(np.int64)).cuda()):
        assert torch.equal(tensor_ops.blend_region(tgx, tgy, tcan, m, 20, solver=solver),
                           tensor_ops.blend_region(tgx, tgy, tcan, mask, 20, solver=solver))
        for mixed in (False, True):
            assert torch.equal(tensor_ops.seamless_clone(tsrc, tcan, m, 20, mixed=mixed, solver=solver),
                               tensor_ops.seamless_clone(tsrc, tcan, mask, 20, mixed=mixed, solver=solver))
