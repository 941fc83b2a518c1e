"""The numpy model of ccp_grid_irls_adjoint_step_device (include/ccp_gs.h, "Differentiating IRLS at its fixed point") and
of the loop tensor_ops.WeightedSolver.fixed_point_grad runs with it, NOT product code.

* `step`: one fused step in the header's operation order -- adjoint_helpers.gradients' wx, wy (lam) of (v, u), then
  reweight_adjoint_helpers.vjp's g_u of those, G + g_u, and ccp_grid_adjoint_begin_device's masking -- so that the kernel
  compares bit for bit; and the report's two sums per channel.
* `fixed_point_gradients`: the z iteration z_0 = G, z_{k+1} = G + J'z_k at a given u with exact (dense) adjoint solves, or
  with `adjoint` replaced (the numpy PCG model: `pcg_hooks`), and the parameter gradients taken once after the last step.
* `dense_fixed_point_gradients`: the forward loop (reweight_adjoint_helpers.dense_unrolled) and then the above."""
import math

import numpy as np

import adjoint_helpers as ah
import constrained_helpers as ch
import reweight_adjoint_helpers as rah
import reweight_helpers as rh
import robust_helpers as bh

NAMES = ("f", "gx", "gy", "values", "base_wx", "base_wy", "data_weight")


def _sets(a, H, W, S):
    """an optional H x W (x S) array as H x W x S (None stays None)"""
    if a is None:
        return None
    a = np.asarray(a)
    return np.broadcast_to(a[..., None] if a.ndim == 2 else a, (H, W, S))


def upstream(v, u, gx=None, gy=None, data=None, fixed=None, per_channel=False):
    """(Gwx, Gwy, Glambda) as ccp_grid_weighted_adjoint_device forms g_wx, g_wy, g_lambda from (v, u): H x W on a shared
    operator, H x W x C (channel c from channel c alone) on one per channel; Glambda None without `data`."""
    u = rh._wide(u)
    H, W, C = u.shape
    f = None if data is None else rh._wide(data.get("f"), u.shape)
    if not per_channel:
        g = ah.gradients(v, u, None, gx, gy, f, fixed=fixed)
        return g["wx"], g["wy"], (g["lam"] if data is not None else None)
    fx = _sets(fixed, H, W, C)
    one = lambda a, c: None if a is None else np.asarray(a)[:, :, c:c + 1]
    gs = [ah.gradients(np.asarray(v)[:, :, c:c + 1], u[:, :, c:c + 1], None, one(gx, c), one(gy, c), one(f, c),
                       fixed=None if fx is None else fx[:, :, c]) for c in range(C)]
    stack = lambda n: np.stack([g[n] for g in gs], axis=-1)
    return stack("wx"), stack("wy"), (stack("lam") if data is not None else None)


def step(v, z_old, u, G, penalty, coupling, scale, eps, gx=None, gy=None, base_wx=None, base_wy=None, per_channel=False, data=None,
         fixed=None, live=None):
    """(b, report, z) after one fused step.  v: the handle's x (H x W x C), z_old: its b, u: the fixed point, G: dL/du.
    The reweight's arguments as reweight_adjoint_helpers.vjp takes them; fixed: the mask (H x W, or H x W x C per channel);
    live: d != 0 of the installed operator, shaped as the mask (None: every pixel that is not fixed).  b: z = G + g_u on
    the free live pixels, +0.0 elsewhere; report: C x 2, (sum (b - z_old)^2, sum b^2) over channel c's free live pixels,
    each the exactly rounded sum (math.fsum) of the float64 squares; z: G + g_u at every pixel, fixed ones included."""
    u = rh._wide(u)
    H, W, C = u.shape
    S = C if per_channel else 1
    Gwx, Gwy, Gl = upstream(v, u, gx, gy, data, fixed, per_channel)
    back = rah.vjp(u, gx, gy, penalty, coupling, scale, eps, base_wx, base_wy, per_channel, Gwx, Gwy, data, Gl)
    z = rh._wide(G) + back["g_u"]
    fx = np.zeros((H, W, S), bool) if fixed is None else (_sets(fixed, H, W, S) != 0)
    keep = ~fx if live is None else (_sets(live, H, W, S) & ~fx)
    keep = np.broadcast_to(keep, (H, W, C))
    b = np.where(keep, z, 0.0)
    dz = b - np.asarray(z_old, dtype=np.float64)
    report = np.array([[math.fsum((dz[:, :, c] * dz[:, :, c])[keep[:, :, c]]), math.fsum((b[:, :, c] * b[:, :, c])[keep[:, :, c]])]
                       for c in range(C)])
    return b, report, z


def operator_at(u, f, gx, gy, penalty, coupling, strength, eps, data_weight=1.0, base_wx=None, base_wy=None, data_penalty=None,
                data_eps=None):
    """(wx, wy, lam, data) of the shared operator the reweight installs from u, as dense_unrolled's later steps form it"""
    f = rh._wide(f)
    H, W, _ = f.shape
    lam0 = np.broadcast_to(np.asarray(data_weight, dtype=np.float64), (H, W))
    wx, wy = bh.edge_weights(u, gx, gy, penalty, coupling, strength, eps, base_wx, base_wy)
    if data_penalty is None:
        return wx, wy, lam0, None
    data = dict(f=f, penalty=data_penalty, scale=1.0, eps=data_eps, base=lam0)
    return wx, wy, bh.data_weights(u, f, data_penalty, 1.0, data_eps, base=lam0), data


def fixed_point_gradients(u, grad, f, gx, gy, penalty, coupling, strength, eps, backward_steps, data_weight=1.0, base_wx=None,
                          base_wy=None, values=None, fixed=None, data_penalty=None, data_eps=None, adjoint=None):
    """The loop of WeightedSolver.fixed_point_grad's backward at u, on a shared operator: v_0 = A^-1 G; `backward_steps`
    times (z := G + J'z from v, then v := A^-1 z); then the gradient pass and the reweight adjoint once.  adjoint:
    adjoint_helpers.dense_adjoint's replacement (grad, wx, wy, lam, fixed).  Returns (gradients, history): NAMES -> array,
    and per step (||z_new - z_old||, ||z_new||) over all channels' free live pixels."""
    adjoint = adjoint or ah.dense_adjoint
    u = rh._wide(u)
    H, W, C = u.shape
    G = np.asarray(grad, dtype=np.float64)
    wx, wy, lam, data = operator_at(u, f, gx, gy, penalty, coupling, strength, eps, data_weight, base_wx, base_wy, data_penalty, data_eps)
    live = ch.level0(W, H, wx, wy, lam, fixed).live
    z, _ = ah.begin(live, fixed, G)
    v = adjoint(z, wx, wy, lam, fixed)
    history = []
    for _ in range(backward_steps):
        z_new, report, _ = step(v, z, u, G, penalty, coupling, strength, eps, gx, gy, base_wx, base_wy, False, data, fixed, live)
        history.append((math.sqrt(report[:, 0].sum()), math.sqrt(report[:, 1].sum())))
        z = z_new
        v = adjoint(z, wx, wy, lam, fixed)
    got = ah.gradients(v, u, None, gx, gy, f, wx, wy, lam, fixed)
    back = rah.vjp(u, gx, gy, penalty, coupling, strength, eps, base_wx, base_wy, False, got["wx"], got["wy"], data,
                   got["lam"] if data is not None else None)
    z_all = G + back["g_u"]                                  # z at every pixel: the fixed ones' feeds d/dvalues
    out = {"gx": got["gx"] + back["g_gx"], "gy": got["gy"] + back["g_gy"], "base_wx": back["g_base_wx"], "base_wy": back["g_base_wy"],
           "values": ah.gradients(v, u, z_all, gx, gy, f, wx, wy, lam, fixed)["values"]}
    if data is None:
        out.update(f=got["f"], data_weight=got["lam"])
    else:
        out.update(f=got["f"] + back["g_f"], data_weight=back["g_lambda"])
    return out, history


def dense_fixed_point_gradients(grad, f, gx, gy, penalty, coupling, strength, eps, outer, backward_steps, solve=None, adjoint=None, **kw):
    """irls_solve's loop with exact inner solves for `outer` steps (reweight_adjoint_helpers.dense_unrolled; solve: its
    replacement of dense_solve), then fixed_point_gradients at its last iterate.  kw: data_weight, base_wx, base_wy, values,
    fixed, data_penalty, data_eps (first_step is dense_unrolled's default).  Returns (u, gradients, info): info holds the
    forward loop's last update max |u_K - u_{K-1}| and the z iteration's history."""
    iterates, _ = rah.dense_unrolled(f, gx, gy, penalty, coupling, strength, eps, outer, solve=solve, **kw)
    u = iterates[-1]
    update = float(np.abs(u - (iterates[-2] if outer >= 2 else rh._wide(f))).max())
    grads, history = fixed_point_gradients(u, grad, f, gx, gy, penalty, coupling, strength, eps, backward_steps, adjoint=adjoint, **kw)
    return u, grads, dict(forward_update=update, history=history)


def pcg_hooks(tol, kind="rescaled", max_iteration=200):
    """dict(solve=, adjoint=) for dense_fixed_point_gradients: every solve by constrained_helpers.pcg, the numpy model of
    the device's multigrid PCG, channel by channel to sqrt(r'r) < tol * |b_c| -- the forward ones warm-started from the
    previous step's solution (the first from f), the adjoint ones from the previous v (the first from 0), as
    irls_solve_implicit runs them."""
    state = {"u": None, "v": None}

    def run(levels, b, x0):
        x, _, ok, _ = ch.pcg(levels, b, tol * float(np.sqrt(np.sum(b * b))), max_iteration, 2, x0, kind)
        assert ok, "the model's solve did not converge"
        return x

    def solve(gx, gy, f, wx, wy, lam, values, fixed, shape):
        H, W, C = shape
        levels = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
        lv = levels[0]
        fa, va = ah._hwc(f, H, W, C), ah._hwc(values, H, W, C)
        start = fa if state["u"] is None else state["u"]
        u = np.zeros(shape)
        for c in range(C):
            b = ch.rhs(lv, None if gx is None else gx[..., c], None if gy is None else gy[..., c], fa[..., c], va[..., c])
            u[..., c] = run(levels, b, ch.x_after(lv, start[..., c], fa[..., c], va[..., c], init=False))
        state["u"] = u
        return u

    def adjoint(z, wx, wy, lam, fixed):
        H, W, C = z.shape
        levels = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
        v = np.zeros(z.shape)
        for c in range(C):
            v[..., c] = run(levels, z[..., c], None if state["v"] is None else state["v"][..., c])
        state["v"] = v
        return v

    return dict(solve=solve, adjoint=adjoint)


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
EPS, DEPS, STRENGTH, NOISE = 5e-2, 5e-2, 0.1, 0.02
KINK = 1e-5                                                  # a Huber case keeps every |sqrt(q) - eps| at least this far away

# name -> (penalty, coupling, robust data term, base weights and a fixed mask, seed)
CASES = {"tv": ("charbonnier", "pixel", False, True, 4), "tv_l1": ("charbonnier", "pixel", True, True, 3),
         "huber": ("huber", "edge", False, True, 2)}


def case_inputs(name, W, H, C=2):
    """f, float32 guidance of noise NOISE, G, a lambda plane, base weights, and three fixed pixels with their values"""
    _, _, _, full, seed = CASES[name]
    r = np.random.default_rng(seed)
    a = dict(f=rh.step_image(W, H, C, seed, noise=0.05), gx=(NOISE * r.standard_normal((H, W, C))).astype(np.float32),
             gy=(NOISE * r.standard_normal((H, W, C))).astype(np.float32), G=r.standard_normal((H, W, C)), lam=r.uniform(0.75, 1.5, (H, W)),
             wx=r.uniform(0.5, 1.5, (H, W)), wy=r.uniform(0.5, 1.5, (H, W)), values=None, fixed=None)
    if full:
        fixed = np.zeros(H * W, np.uint8)
        fixed[r.choice(H * W, 3, replace=False)] = 1
        a.update(values=r.uniform(0.0, 1.0, (H, W, C)), fixed=fixed.reshape(H, W))
    return a


def case_kw(name, a):
    """the keyword arguments of dense_fixed_point_gradients / dense_unrolled_gradients for case `name` on inputs `a`"""
    _, _, robust, _, _ = CASES[name]
    kw = dict(data_weight=a["lam"], base_wx=a["wx"], base_wy=a["wy"], values=a["values"], fixed=a["fixed"])
    if robust:
        kw.update(data_penalty="charbonnier", data_eps=DEPS)
    return kw


def relative_gap(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


# forward steps to an update <= 1e-12 and backward steps to ||z_new - z_old|| <= 1e-12 ||G|| on case_inputs(name, 16, 12), with
# exact solves (tests/test_fixed_point_helpers.py asserts them); the GPU tests add MARGIN to each
STEPS = {"tv": (35, 36), "tv_l1": (19, 16), "huber": (49, 50)}
MARGIN = 5
