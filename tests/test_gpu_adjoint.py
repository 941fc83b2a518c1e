"""GPU: the backward pass of a weighted solve (include/ccp_gs.h, "Differentiating a weighted solve").

1. ccp_grid_weighted_adjoint_device against tests/adjoint_helpers.py, bit for bit, with x and u seeded random planes;
2. ccp_grid_adjoint_begin_device: the bits of b and x, and the MG-PCG that follows;
3. tensor_ops.weighted_solve_grad end to end against the dense implicit-gradient reference, in every multigrid mode;
4. torch.autograd.gradcheck;  5. autograd behaviour;  6. refusals.

The end-to-end tolerance is not a chosen number: the numpy model of the same PCG (constrained_helpers.pcg) runs both
solves on the CPU to the same epsilon, its gradients' max-norm distance from the dense reference is the figure, and the
device is allowed 16 times that per gradient -- the margin for a different but equally valid rounding path.  Measured
on an MI355X (device distance / model distance, the largest over the seven gradients): see NOTES R20.1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adjoint_helpers as ah
import constrained_helpers as ch
from coursecomputationalphotography_amd import capi, tensor_ops

pytestmark = pytest.mark.gpu

BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6
DEV = "cuda:0"
NAMES = ah.PLANES + ah.IMAGES
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (33, 17), (70, 40), (257, 131)]


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    word = np.uint64 if got.dtype == np.float64 else np.uint32
    return np.array_equal(got.view(word), want.view(word))


def fixed_set(kind, W, H, seed):
    """none / ten: about 10 % of the pixels, with runs and pixels on the canvas border / all."""
    m = np.zeros((H, W), bool)
    if kind == "all":
        m[:] = True
    elif kind == "ten":
        m = rng(seed).uniform(size=(H, W)) < 0.1
        m[0, : max(1, W // 3)] = True                        # a run along the top border
        m[H // 2:, W - 1] = True                             # a run down the right border
        m[H // 2, W // 4: W // 4 + 3] = True                 # a run inside
    return m


def kernel_case(W, H, Cn, kind, seed):
    """Inputs of one kernel comparison (numpy): random weights with zeros and, where the canvas has room, a block of dead
    pixels (free, lambda = 0, all four weights 0); x and u random, not solved."""
    r = rng(seed)
    p = dict(wx=r.uniform(0.0, 4.0, (H, W)), wy=r.uniform(0.0, 4.0, (H, W)), lam=r.uniform(0.0, 0.3, (H, W)),
             gx=r.uniform(-60, 60, (H, W, Cn)).astype(np.float32), gy=r.uniform(-60, 60, (H, W, Cn)).astype(np.float32),
             f=r.uniform(0, 255, (H, W, Cn)))
    p["wx"][r.uniform(size=(H, W)) < 0.1] = 0.0
    p["wy"][r.uniform(size=(H, W)) < 0.1] = 0.0
    fixed = fixed_set(kind, W, H, seed + 1)
    if W >= 6 and H >= 6 and kind != "all":
        y0, x0 = H // 2 + 1, W // 2
        p["lam"][y0:y0 + 2, x0:x0 + 2] = 0.0
        p["wx"][y0:y0 + 2, x0 - 1:x0 + 2] = 0.0
        p["wy"][y0 - 1:y0 + 2, x0:x0 + 2] = 0.0
        fixed[y0:y0 + 2, x0:x0 + 2] = False
        assert not ch.level0(W, H, p["wx"], p["wy"], p["lam"], fixed).live[y0:y0 + 2, x0:x0 + 2].any()
    x, u, G = r.uniform(-3, 3, (H, W, Cn)), r.uniform(-2, 2, (H, W, Cn)), r.uniform(-1, 1, (H, W, Cn))
    return p, fixed, x, u, G


def handle(W, H, Cn, p, fixed, x=None):
    g = capi.Grid(W, H, Cn, weighted=True)
    g.set_weights_tensor(dev(p.get("wx")), dev(p.get("wy")), dev(p.get("lam")), fixed=None if fixed is None else dev(fixed))
    if x is not None:
        g.set_x_tensor(dev(x))
    return g


def check_outputs(got, want, dtype=np.float64, names=NAMES):
    assert sorted(got) == sorted(names)
    for n in names:
        assert bits_equal(got[n].cpu().numpy(), want[n].astype(dtype)), n


# ---- 1. the kernel against the model, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "ten", "all"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_kernel_matches_the_model_bit_for_bit(W, H, Cn, kind):
    p, fixed, x, u, G = kernel_case(W, H, Cn, kind, 100 + 7 * W + H + Cn)
    want = ah.gradients(x, u, G, fixed=fixed, **p)
    g = handle(W, H, Cn, p, fixed, x)
    t = {k: dev(a) for k, a in p.items()}
    args = (dev(u), dev(G), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], dev(fixed))
    check_outputs(g.weighted_adjoint_tensor(*args), want)
    check_outputs(g.weighted_adjoint_tensor(*args, dtype=torch.float32), want, np.float32)      # rounded once
    # x at the fixed pixels is read as 0 whatever it holds
    g.set_x_tensor(dev(np.where(fixed[..., None], 1e3, x)))
    check_outputs(g.weighted_adjoint_tensor(*args), want)
    g.close()


@pytest.mark.parametrize("W,H,Cn", [(33, 17, 3), (70, 40, 1), (2, 2, 3), (1, 7, 1)])
def test_absent_inputs_and_input_dtypes(W, H, Cn):
    """NULL gx / gy / f / wx / lambda read 0 / 0 / 0 / 1 / 0; float32 weights and grad, u8 f, a float32 mask, no mask."""
    p, fixed, x, u, G = kernel_case(W, H, Cn, "ten", 300 + W)
    g = handle(W, H, Cn, p, fixed, x)
    for drop in (("gx", "gy", "f", "wx", "lam"), ("gx",), ("gy", "wy"), ("f", "lam")):
        q = {k: (None if k in drop else a) for k, a in p.items()}
        want = ah.gradients(x, u, G, fixed=fixed, **q)
        t = {k: dev(a) for k, a in q.items()}
        got = g.weighted_adjoint_tensor(dev(u), dev(G), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], dev(fixed))
        check_outputs(got, want)
    q = dict(p, wx=p["wx"].astype(np.float32), wy=p["wy"].astype(np.float32), lam=p["lam"].astype(np.float32),
             f=np.floor(p["f"]).astype(np.uint8))
    G32 = G.astype(np.float32)
    t = {k: dev(a) for k, a in q.items()}
    for mask in (dev(fixed), dev(fixed.astype(np.float32)), dev(fixed.astype(np.uint8))):
        got = g.weighted_adjoint_tensor(dev(u), dev(G32), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], mask)
        check_outputs(got, ah.gradients(x, u, G32, fixed=fixed, **q))
    got = g.weighted_adjoint_tensor(dev(u), dev(G), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], None)
    check_outputs(got, ah.gradients(x, u, G, fixed=None, **q))
    g.close()


def test_broadcast_scalar_weights():
    W, H, Cn = 33, 17, 3
    p, fixed, x, u, G = kernel_case(W, H, Cn, "ten", 41)
    p.update(wx=np.full((H, W), 2.5), wy=np.full((H, W), 0.75), lam=np.full((H, W), 0.125))
    g = handle(W, H, Cn, p, fixed, x)
    scalar = {k: torch.tensor(float(p[k][0, 0]), dtype=torch.float64, device=DEV).expand(H, W) for k in ("wx", "wy", "lam")}
    got = g.weighted_adjoint_tensor(dev(u), dev(G), dev(p["gx"]), dev(p["gy"]), dev(p["f"]), scalar["wx"], scalar["wy"],
                                    scalar["lam"], dev(fixed))
    check_outputs(got, ah.gradients(x, u, G, fixed=fixed, **p))
    g.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_non_contiguous_outputs_and_requested_subsets(dtype):
    """A planar view; a sub-window of a larger tensor whose surroundings keep their bits; only some outputs asked for."""
    W, H, Cn = 70, 40, 3
    p, fixed, x, u, G = kernel_case(W, H, Cn, "ten", 77)
    want = ah.gradients(x, u, G, fixed=fixed, **p)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    g = handle(W, H, Cn, p, fixed, x)
    t = {k: dev(a) for k, a in p.items()}
    args = (dev(u), dev(G), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], dev(fixed))
    planar = {n: torch.empty((Cn, H, W), dtype=dtype, device=DEV).permute(1, 2, 0) for n in ah.IMAGES}
    planar.update({n: torch.empty((W, H), dtype=dtype, device=DEV).t() for n in ah.PLANES})
    check_outputs(g.weighted_adjoint_tensor(*args, out=planar), want, np_dtype)
    big = {n: torch.full((H + 5, W + 7, Cn + 1), -7.0, dtype=dtype, device=DEV) for n in ah.IMAGES}
    big.update({n: torch.full((H + 5, W + 7), -7.0, dtype=dtype, device=DEV) for n in ah.PLANES})
    window = {n: (b[2:2 + H, 3:3 + W, :Cn] if b.dim() == 3 else b[2:2 + H, 3:3 + W]) for n, b in big.items()}
    check_outputs(g.weighted_adjoint_tensor(*args, out=window), want, np_dtype)
    for n, b in big.items():
        rest = b.clone()
        (rest[2:2 + H, 3:3 + W, :Cn] if b.dim() == 3 else rest[2:2 + H, 3:3 + W]).fill_(-7.0)
        assert bool((rest == -7.0).all()), f"{n}: the surroundings of the window changed"
    for names in (("wx",), ("f", "values"), ("lam", "gy"), ("gx", "wy")):
        got = g.weighted_adjoint_tensor(*args, want=names, dtype=dtype)
        check_outputs(got, want, np_dtype, names)
    # without the gradient of values, grad is not needed
    got = g.weighted_adjoint_tensor(dev(u), None, *args[2:], want=("wx", "f"), dtype=dtype)
    check_outputs(got, want, np_dtype, ("wx", "f"))
    g.close()


# ---- 2. adjoint_begin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("W,H,Cn,kind", [(33, 17, 2, "ten"), (70, 40, 3, "ten"), (7, 1, 1, "none"), (1, 1, 1, "none"), (2, 2, 3, "all")])
def test_adjoint_begin_bits_and_the_solve_that_follows(W, H, Cn, kind, grad_dtype):
    p, fixed, x, _, G = kernel_case(W, H, Cn, kind, 900 + W)
    p["lam"] = np.where(p["lam"] == 0.0, 0.0, p["lam"] + 0.05)        # screened, and the dead block stays dead
    G = G.astype(grad_dtype)
    g = handle(W, H, Cn, p, fixed, x)
    g.mg_set_hierarchy("rescaled")
    g.set_b_tensor(dev(np.full((H, W, Cn), 7.0)))
    lv = ch.level0(W, H, p["wx"], p["wy"], p["lam"], fixed)
    g.adjoint_begin_tensor(dev(G))
    b, x0 = ah.begin(lv.live, fixed, G)
    assert bits_equal(g.get_b_tensor().cpu().numpy(), b)
    assert bits_equal(g.get_x_tensor().cpu().numpy(), x0)
    eps = 1e-10 * max(float(np.sqrt(np.sum(b * b))), 1e-300)
    reports = g.mg_conjugate_gradient(eps, 200, 2)
    assert all(r.converged for r in reports), [(r.iterations, r.last_l1_step) for r in reports]
    v = g.get_x_tensor().cpu().numpy()
    assert not v[fixed].any() and not v[~lv.live].any()
    if lv.live.any():
        want = ah.dense_adjoint(b, p["wx"], p["wy"], p["lam"], fixed)
        assert np.abs(v - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-300)
    g.close()


# ---- 3. end to end against the dense reference ------------------------------------------------------------------------------
def e2e_problem(W, H, Cn, seed):
    r = rng(seed)
    p = dict(gx=r.uniform(-1, 1, (H, W, Cn)).astype(np.float32), gy=r.uniform(-1, 1, (H, W, Cn)).astype(np.float32),
             f=r.uniform(0, 1, (H, W, Cn)), wx=r.uniform(0.1, 10, (H, W)), wy=r.uniform(0.1, 10, (H, W)),
             lam=np.full((H, W), 1e-2), values=r.uniform(0, 1, (H, W, Cn)))
    fixed = r.uniform(size=(H, W)) < 0.1
    G = r.uniform(-1, 1, (H, W, Cn))
    return p, fixed, G


@functools.lru_cache(maxsize=None)
def e2e_reference(W, H, Cn):
    """The problem, the dense reference's gradients, the model's distance from them per gradient, and epsilon -- computed
    once per shape and shared by every mode."""
    p, fixed, G = e2e_problem(W, H, Cn, 500 + W)
    _, _, ref = ah.dense_reference(G, fixed=fixed, **p)
    _, _, model, eps = ah.pcg_gradients(G, 1e-12, fixed=fixed, **p)
    return p, fixed, G, ref, {n: float(np.abs(model[n] - ref[n]).max()) for n in NAMES}, eps


def device_gradients(p, fixed, G, eps, **mode):
    t = {k: dev(a) for k, a in p.items()}
    for k in t:
        t[k].requires_grad_(True)
    x = tensor_ops.weighted_solve_grad(t["gx"], t["gy"], t["f"], 200, wx=t["wx"], wy=t["wy"], data_weight=t["lam"],
                                       values=t["values"], fixed=dev(fixed), epsilon=eps, hierarchy="rescaled", **mode)
    assert x.dtype == torch.float64 and x.grad_fn is not None
    (dev(G) * x).sum().backward()
    return x.detach().cpu().numpy(), {("lam" if k == "lam" else k): t[k].grad.cpu().numpy() for k in t}


MODES = {"sequential": {}, "batched": dict(channels="batched"), "f32": dict(precision="f32"), "line": dict(smoother="line")}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H,Cn", [(33, 17, 2), (70, 40, 3)])
def test_end_to_end_against_the_dense_reference(W, H, Cn, mode):
    p, fixed, G, ref, model_distance, eps = e2e_reference(W, H, Cn)
    x, got = device_gradients(p, fixed, G, eps, **MODES[mode])
    assert got["gx"].dtype == np.float32 and got["wx"].dtype == np.float64
    worst = {}
    for n in NAMES:
        worst[n] = float(np.abs(got[n].astype(np.float64) - ref[n]).max())
        print(f"{W}x{H}x{Cn} {mode} d/d{n}: device {worst[n]:.3e}  model {model_distance[n]:.3e}  max|ref| {np.abs(ref[n]).max():.3e}")
    for n in NAMES:
        if got[n].dtype == np.float64:
            assert worst[n] <= 16 * model_distance[n], (n, worst[n], model_distance[n])
        else:
            # gx and gy are float32 inputs, so autograd's gradient is the fp64 value rounded to float32 once: on top of the
            # fp64 bound each element may be half a float32 ulp away.  (The fp64 values themselves: the sequential case below.)
            half_ulp = 0.5 * np.spacing(np.abs(ref[n]).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got[n].astype(np.float64) - ref[n]) <= 16 * model_distance[n] + half_ulp), n
    if mode == "sequential":
        # the same chain by hand with every gradient in fp64: gx and gy meet the bound with no allowance, and autograd
        # returned exactly these values (the float32 ones rounded once)
        g = handle(W, H, Cn, p, fixed)
        g.mg_set_hierarchy("rescaled")
        t = {k: dev(a) for k, a in p.items()}
        g.assemble_constrained_rhs_tensor(t["gx"], t["gy"], t["f"], t["values"], init_x=True)
        assert all(r.converged for r in g.mg_conjugate_gradient(eps, 200, 2))
        u = g.get_x_tensor()
        assert bits_equal(u.cpu().numpy(), x)
        g.adjoint_begin_tensor(dev(G))
        assert all(r.converged for r in g.mg_conjugate_gradient(eps, 200, 2))
        wide = g.weighted_adjoint_tensor(u, dev(G), t["gx"], t["gy"], t["f"], t["wx"], t["wy"], t["lam"], dev(fixed))
        g.close()
        for n in NAMES:
            w = wide[n].cpu().numpy()
            assert float(np.abs(w - ref[n]).max()) <= 16 * model_distance[n], (n, float(np.abs(w - ref[n]).max()), model_distance[n])
            assert bits_equal(got[n], w.astype(got[n].dtype)), n
    if mode == "batched":
        xs, gs = device_gradients(p, fixed, G, eps)
        assert bits_equal(x, xs)
        for n in NAMES:
            assert bits_equal(got[n], gs[n]), n


# ---- 4. gradcheck ----------------------------------------------------------------------------------------------------------
def test_gradcheck():
    W, H = 6, 5
    r = rng(64)
    gx, gy = dev(r.uniform(-1, 1, (H, W, 1)).astype(np.float32)), dev(r.uniform(-1, 1, (H, W, 1)).astype(np.float32))
    fixed = r.uniform(size=(H, W)) < 0.2
    ins = [dev(r.uniform(0.1, 10, (H, W))), dev(r.uniform(0.1, 10, (H, W))), dev(r.uniform(0.01, 1, (H, W))),
           dev(r.uniform(0, 1, (H, W, 1))), dev(r.uniform(0, 1, (H, W, 1)))]
    lv = ch.level0(W, H, ins[0].cpu().numpy(), ins[1].cpu().numpy(), ins[2].cpu().numpy(), fixed)
    b = ch.rhs(lv, gx.cpu().numpy()[..., 0], gy.cpu().numpy()[..., 0], ins[3].cpu().numpy()[..., 0], ins[4].cpu().numpy()[..., 0])
    eps = 1e-13 * float(np.sqrt(np.sum(b * b)))
    for t in ins:
        t.requires_grad_(True)
    mask = dev(fixed)

    def solve(wx, wy, lam, f, values):
        return tensor_ops.weighted_solve_grad(gx, gy, f, 200, wx=wx, wy=wy, data_weight=lam, values=values, fixed=mask, epsilon=eps)

    assert torch.autograd.gradcheck(solve, ins)


# ---- 5. autograd behaviour -------------------------------------------------------------------------------------------------
def small_problem(seed=5, W=33, H=17, Cn=2):
    p, fixed, G = e2e_problem(W, H, Cn, seed)
    p["lam"] = np.full((H, W), 0.05)
    return {k: dev(a) for k, a in p.items()}, dev(fixed), dev(G)


def solve(t, fixed, **kw):
    kw.setdefault("epsilon", 1e-9)
    return tensor_ops.weighted_solve_grad(t["gx"], t["gy"], t["f"], 200, wx=t["wx"], wy=t["wy"], data_weight=t["lam"], values=t["values"],
                                          fixed=fixed, **kw)


def test_backward_twice_with_retain_graph_and_the_handle_lifetime(monkeypatch):
    closed = []
    real_close = capi.Grid.close
    monkeypatch.setattr(capi.Grid, "close", lambda self: (closed.append(bool(self.h)), real_close(self))[1])
    t, fixed, G = small_problem()
    for k in ("wx", "f", "values", "gx"):
        t[k].requires_grad_(True)
    wanted = [t[k] for k in ("wx", "f", "values", "gx")]
    x = solve(t, fixed)
    loss = (G * x).sum()
    first = torch.autograd.grad(loss, wanted, retain_graph=True)
    assert not any(closed)                                   # the handle is alive: the graph was retained
    second = torch.autograd.grad(loss, wanted)
    for a, b in zip(first, second):
        assert bits_equal(a.cpu().numpy(), b.cpu().numpy())
    assert closed.count(True) == 1                           # released with the node's saved tensors
    with pytest.raises(RuntimeError):
        torch.autograd.grad(loss, wanted)
    # a graph dropped without a backward releases the handle too
    closed.clear()
    x = solve(t, fixed)
    assert not any(closed)
    del x
    assert closed.count(True) == 1


def test_scalar_weights_get_the_sum_of_the_planes_gradient():
    t, fixed, G = small_problem(6)
    H, W = fixed.shape
    planes = {}
    for k, value in (("wx", 1.7), ("lam", 0.05)):
        t[k] = torch.full((H, W), value, dtype=torch.float64, device=DEV, requires_grad=True)
    (G * solve(t, fixed)).sum().backward()
    planes = {k: t[k].grad for k in ("wx", "lam")}
    s = dict(t)
    s["wx"] = torch.tensor(1.7, dtype=torch.float64, device=DEV, requires_grad=True)
    s["lam"] = torch.tensor(0.05, dtype=torch.float64, device=DEV, requires_grad=True)
    (G * solve(s, fixed)).sum().backward()
    for k in ("wx", "lam"):
        assert s[k].grad.shape == ()
        # the same terms summed in another order: n * 2^-53 of the sum of magnitudes, n = H * W
        assert abs(float(s[k].grad) - float(planes[k].sum())) <= 1e-12 * float(planes[k].abs().sum()), k
    # a python scalar is a constant
    s["wx"], s["lam"] = 1.7, 0.05
    s["f"].requires_grad_(True)
    x = solve(s, fixed)
    (G * x).sum().backward()
    assert s["f"].grad is not None


def test_only_the_requested_gradients_are_computed(monkeypatch):
    asked = []
    real = capi.Grid.weighted_adjoint_tensor

    def spy(self, *a, **kw):
        asked.append(tuple(kw["want"]))
        return real(self, *a, **kw)

    monkeypatch.setattr(capi.Grid, "weighted_adjoint_tensor", spy)
    set_weights = []
    real_set = capi.Grid.set_weights_tensor
    monkeypatch.setattr(capi.Grid, "set_weights_tensor", lambda self, *a, **kw: (set_weights.append(1), real_set(self, *a, **kw))[1])
    t, fixed, G = small_problem(7)
    t["f"] = (t["f"] * 255).to(torch.uint8)                  # a u8 input gets no gradient
    t["wy"].requires_grad_(True)
    t["values"].requires_grad_(True)
    (G * solve(t, fixed)).sum().backward()
    assert asked == [("wy", "values")]
    assert len(set_weights) == 1                             # backward never forms the operator again
    assert t["wy"].grad is not None and t["values"].grad is not None
    assert all(t[k].grad is None for k in ("gx", "gy", "f", "wx", "lam"))
    assert t["wy"].grad.dtype == torch.float64 and t["wy"].grad.shape == t["wy"].shape


def test_strict_raises_when_a_solve_does_not_converge():
    t, fixed, G = small_problem(8)
    t["wx"].requires_grad_(True)
    with pytest.raises(RuntimeError, match="did not converge"):
        tensor_ops.weighted_solve_grad(t["gx"], t["gy"], t["f"], 1, wx=t["wx"], wy=t["wy"], data_weight=t["lam"], values=t["values"],
                                       fixed=fixed, epsilon=1e-12)
    x = tensor_ops.weighted_solve_grad(t["gx"], t["gy"], t["f"], 1, wx=t["wx"], wy=t["wy"], data_weight=t["lam"], values=t["values"],
                                       fixed=fixed, epsilon=1e-12, strict=False)
    (G * x).sum().backward()                                 # not the gradient, but no error either
    assert t["wx"].grad is not None


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def darr(t, code=None):
    codes = {torch.uint8: capi.DTYPE_U8, torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    s = list(t.stride()) + [0] * (3 - t.dim())
    return capi.DeviceArray(t.data_ptr(), codes[t.dtype] if code is None else code, 0, 0, s[0], s[1], s[2])


def raw_adjoint(g, ins, outs):
    a = capi.AdjointInputs(*[C.pointer(darr(ins[n])) if n in ins else None for n in capi.ADJOINT_INPUTS])
    b = capi.AdjointOutputs(*[C.pointer(darr(outs[n])) if n in outs else None for n in capi.ADJOINT_OUTPUTS])
    return g.L.ccp_grid_weighted_adjoint_device(g.h, C.byref(a), C.byref(b))


def raw_begin(g, grad):
    return g.L.ccp_grid_adjoint_begin_device(g.h, C.byref(darr(grad)))


def test_refusals_leave_everything_untouched():
    W, H, Cn = 9, 6, 2
    ones = lambda *shape, dtype=torch.float64: torch.full(shape, 5.0, dtype=dtype, device=DEV)
    u, grad = ones(H, W, Cn), ones(H, W, Cn)
    outs = lambda: {"g_wx": ones(H, W), "g_lambda": ones(H, W), "g_gx": ones(H, W, Cn), "g_values": ones(H, W, Cn)}

    def untouched(g, o):
        torch.cuda.synchronize()
        assert all(bool((t == 5.0).all()) for t in o.values())
        for c in range(Cn):
            assert np.all(g.get_x(c) == 3.0) and np.all(g.get_b(c) == 4.0)

    def prepared(g):
        g.fill_x(3.0)
        for c in range(Cn):
            g.set_b(np.full((H, W), 4.0), c)
        return g

    mask = np.ones((H, W), np.uint8)
    for g in (prepared(capi.Grid(W, H, Cn)), prepared(capi.Grid(W, H, Cn, mask=mask))):       # structured, Dirichlet mask
        o = outs()
        assert raw_adjoint(g, {"u": u, "grad_x": grad}, o) == UNSUPPORTED
        assert raw_begin(g, grad) == UNSUPPORTED
        untouched(g, o)
        g.close()
    g = prepared(capi.Grid(W, H, Cn, weighted=True))
    o = outs()
    assert raw_adjoint(g, {"u": u, "grad_x": grad}, o) == STATE                             # no operator yet
    assert raw_begin(g, grad) == STATE
    untouched(g, o)
    g.set_weights()
    prepared(g)
    bad = [({"u": ones(H, W, Cn, dtype=torch.float32), "grad_x": grad}, outs()),          # u must be F64
           ({"u": u, "grad_x": ones(H, W, Cn, dtype=torch.uint8)}, outs()),               # grad: F32 or F64
           ({"u": u, "grad_x": grad, "gx": ones(H, W, Cn)}, outs()),                      # gx: F32
           ({"u": u, "grad_x": grad, "wx": ones(H, W, dtype=torch.uint8)}, outs()),       # weights: F32 or F64
           ({"u": u}, outs()),                                                              # g_values without grad
           ({"grad_x": grad}, outs())]                                                      # no u
    o = outs()
    o["g_gx"] = ones(H, W, 1).expand(H, W, Cn)                                              # overlapping output elements
    bad.append(({"u": u, "grad_x": grad}, o))
    o = outs()
    o["g_wx"] = ones(1, W).expand(H, W)
    bad.append(({"u": u, "grad_x": grad}, o))
    o = outs()
    o["g_lambda"] = torch.full((H, W), 5, dtype=torch.uint8, device=DEV)                    # an output dtype that is no float
    bad.append(({"u": u, "grad_x": grad}, o))
    for ins, o in bad:
        assert raw_adjoint(g, ins, o) == BAD_ARG, sorted(ins)
        untouched(g, o)
    assert g.L.ccp_grid_weighted_adjoint_device(g.h, None, None) == BAD_ARG
    assert raw_begin(g, ones(H, W, Cn, dtype=torch.uint8)) == BAD_ARG
    assert raw_begin(g, ones(H, W, 1).expand(H, W, Cn)) == capi.CCP_OK                      # an input may broadcast
    g.close()
