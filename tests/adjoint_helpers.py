"""Test-side expectations of the backward pass of a weighted solve (include/ccp_gs.h, "Differentiating a weighted solve"),
NOT product code.

* `begin` and `gradients`: ccp_grid_adjoint_begin_device and ccp_grid_weighted_adjoint_device in numpy, in the header's
  operation order (fp64, inputs widened exactly, channels accumulated in channel order from +0.0), so that the kernels
  compare bit for bit.  float32 outputs are these values rounded once (`.astype(np.float32)`).
* `dense_solve` / `dense_reference`: the implicit-gradient reference.  The energy's normal equations as a DENSE matrix,
  restricted to the free live pixels, solved by numpy.linalg.solve: the forward composite u, the adjoint solution v, and
  the formulas on those.  tests/test_adjoint_helpers.py checks the formulas against central differences of dense_solve.
* `pcg_gradients`: the same formulas on the u and v of constrained_helpers.pcg, the numpy model of the device's MG-PCG --
  how far an equally valid rounding path lands from the dense reference (the end-to-end tolerance of test_gpu_adjoint).
"""
import numpy as np

import constrained_helpers as ch

PLANES = ("wx", "wy", "lam")
IMAGES = ("gx", "gy", "f", "values")


def _hwc(a, H, W, C, fill=0.0):
    """An H x W x C float64 array: `a` widened exactly (a 2-D array is one channel), or `fill` everywhere."""
    if a is None:
        return np.full((H, W, C), fill, dtype=np.float64)
    a = np.asarray(a)
    return (a if a.ndim == 3 else a[..., None]).astype(np.float64)


def _hw(a, H, W, fill):
    if a is None:
        return np.full((H, W), fill, dtype=np.float64)
    return np.broadcast_to(np.asarray(a).astype(np.float64), (H, W)).copy()


def _fixed(fixed, H, W):
    return np.zeros((H, W), bool) if fixed is None else (np.asarray(fixed) != 0)


def begin(live, fixed, grad):
    """(b, x) after ccp_grid_adjoint_begin_device: b = grad on free live pixels, +0.0 elsewhere; x = +0.0.  live: d != 0
    of the installed operator (constrained_helpers.level0(...).live: a fixed pixel's d is 0)."""
    g = np.asarray(grad)
    g = (g if g.ndim == 3 else g[..., None]).astype(np.float64)
    keep = (np.asarray(live) & ~_fixed(fixed, *g.shape[:2]))[..., None]
    return np.where(keep, g, 0.0), np.zeros_like(g)


def gradients(x, u, grad=None, gx=None, gy=None, f=None, wx=None, wy=None, lam=None, fixed=None):
    """Every output of ccp_grid_weighted_adjoint_device as float64 arrays: {"wx", "wy", "lam"} H x W and {"gx", "gy", "f",
    "values"} H x W x C.  x: the handle's x (H x W x C; read as +0.0 at fixed pixels), u: the forward composite."""
    u = np.asarray(u, dtype=np.float64)
    u = u if u.ndim == 3 else u[..., None]
    H, W, C = u.shape
    fx = _fixed(fixed, H, W)
    v = np.where(fx[..., None], 0.0, _hwc(x, H, W, C))
    G, gx, gy, f = _hwc(grad, H, W, C), _hwc(gx, H, W, C), _hwc(gy, H, W, C), _hwc(f, H, W, C)
    wx, wy, lam = _hw(wx, H, W, 1.0), _hw(wy, H, W, 1.0), _hw(lam, H, W, 0.0)
    out = {n: np.zeros((H, W)) for n in PLANES}
    out.update({n: np.zeros((H, W, C)) for n in IMAGES})
    for c in range(C):
        vc, uc = v[..., c], u[..., c]
        # east edges (x + 1 < W): s = vE - v; r = gx - (uE - u); g_gx = w * s; acc += s * r
        s = vc[:, 1:] - vc[:, :-1]
        r = gx[:, :-1, c] - (uc[:, 1:] - uc[:, :-1])
        out["gx"][:, :-1, c] = wx[:, :-1] * s
        out["wx"][:, :-1] = out["wx"][:, :-1] + s * r
        # south edges (y + 1 < H)
        s = vc[1:, :] - vc[:-1, :]
        r = gy[:-1, :, c] - (uc[1:, :] - uc[:-1, :])
        out["gy"][:-1, :, c] = wy[:-1, :] * s
        out["wy"][:-1, :] = out["wy"][:-1, :] + s * r
        # free pixels: g_f = lambda * v; accl += v * (f - u)
        out["f"][..., c] = np.where(fx, 0.0, lam * vc)
        out["lam"] = np.where(fx, 0.0, out["lam"] + vc * (f[..., c] - uc))
        # fixed pixels: t = G; += wN vN; += wW vW; += wE vE; += wS vS (absent edges skipped)
        t = G[..., c].copy()
        t[1:, :] = t[1:, :] + wy[:-1, :] * vc[:-1, :]
        t[:, 1:] = t[:, 1:] + wx[:, :-1] * vc[:, :-1]
        t[:, :-1] = t[:, :-1] + wx[:, :-1] * vc[:, 1:]
        t[:-1, :] = t[:-1, :] + wy[:-1, :] * vc[1:, :]
        out["values"][..., c] = np.where(fx, t, 0.0)
    return out


# ---- the dense implicit-gradient reference ------------------------------------------------------------------------------
def dense_system(W, H, wx=None, wy=None, lam=None):
    """The energy's Hessian / 2 over ALL pixels as a dense matrix (raster order) and the edge index pairs."""
    wx, wy, lam = _hw(wx, H, W, 1.0), _hw(wy, H, W, 1.0), _hw(lam, H, W, 0.0)
    idx = np.arange(W * H).reshape(H, W)
    A = np.diag(lam.ravel())
    for a, b, w in ((idx[:, :-1], idx[:, 1:], wx[:, :-1]), (idx[:-1, :], idx[1:, :], wy[:-1, :])):
        a, b, w = a.ravel(), b.ravel(), w.ravel()
        np.add.at(A, (a, a), w)
        np.add.at(A, (b, b), w)
        np.add.at(A, (a, b), -w)
        np.add.at(A, (b, a), -w)
    return A


def _unknowns(A, fixed):
    """Raster indices of the free live pixels (a free pixel whose row of A is empty is dead: it keeps 0)."""
    return np.flatnonzero(~fixed.ravel() & (np.diag(A) != 0.0))


def dense_solve(gx=None, gy=None, f=None, wx=None, wy=None, lam=None, values=None, fixed=None, shape=None):
    """The composite u (H x W x C, float64): the energy's minimiser over the free live pixels by numpy.linalg.solve on
    the dense A_FF, `values` on the fixed pixels, 0 on dead free ones."""
    H, W, C = shape
    fx = _fixed(fixed, H, W)
    wxa, wya, lama = _hw(wx, H, W, 1.0), _hw(wy, H, W, 1.0), _hw(lam, H, W, 0.0)
    A = dense_system(W, H, wxa, wya, lama)
    free, fix = _unknowns(A, fx), np.flatnonzero(fx.ravel())
    gx, gy, f, vals = _hwc(gx, H, W, C), _hwc(gy, H, W, C), _hwc(f, H, W, C), _hwc(values, H, W, C)
    u = np.zeros((H, W, C))
    for c in range(C):
        b = lama * f[..., c]
        b[:, :-1] -= wxa[:, :-1] * gx[:, :-1, c]
        b[:, 1:] += wxa[:, :-1] * gx[:, :-1, c]
        b[:-1, :] -= wya[:-1, :] * gy[:-1, :, c]
        b[1:, :] += wya[:-1, :] * gy[:-1, :, c]
        uc = np.zeros(W * H)
        uc[fix] = vals[..., c].ravel()[fix]
        if len(free):
            uc[free] = np.linalg.solve(A[np.ix_(free, free)], b.ravel()[free] - A[np.ix_(free, fix)] @ uc[fix])
        u[..., c] = uc.reshape(H, W)
    return u


def dense_adjoint(grad, wx=None, wy=None, lam=None, fixed=None):
    """v (H x W x C): A_FF v_F = G_F on the free live pixels, 0 elsewhere."""
    G = np.asarray(grad, dtype=np.float64)
    H, W, C = G.shape
    fx = _fixed(fixed, H, W)
    A = dense_system(W, H, wx, wy, lam)
    free = _unknowns(A, fx)
    v = np.zeros((H, W, C))
    if len(free):
        sol = np.linalg.solve(A[np.ix_(free, free)], G.reshape(H * W, C)[free])
        v.reshape(H * W, C)[free] = sol
    return v


def dense_reference(grad, gx=None, gy=None, f=None, wx=None, wy=None, lam=None, values=None, fixed=None):
    """(u, v, gradients) of L = sum grad * u by the implicit-function formulas on the dense solves."""
    u = dense_solve(gx, gy, f, wx, wy, lam, values, fixed, shape=np.asarray(grad).shape)
    v = dense_adjoint(grad, wx, wy, lam, fixed)
    return u, v, gradients(v, u, grad, gx, gy, f, wx, wy, lam, fixed)


def pcg_gradients(grad, epsilon_rel, gx=None, gy=None, f=None, wx=None, wy=None, lam=None, values=None, fixed=None,
                  kind="rescaled", max_iteration=200):
    """The formulas on the numpy model of the device's solves: both systems by constrained_helpers.pcg, channel by
    channel, to the ONE absolute epsilon tensor_ops.weighted_solve_grad would be given -- epsilon_rel * ||b||, b the
    forward right-hand side of all channels -- the forward one from x = f as tensor_ops starts it.  Returns (u, v,
    gradients, epsilon)."""
    G = np.asarray(grad, dtype=np.float64)
    H, W, C = G.shape
    levels = ch.hierarchy(W, H, wx, wy, lam, fixed, kind)
    lv = levels[0]
    fa, va = _hwc(f, H, W, C), _hwc(values, H, W, C)
    u, v = np.zeros((H, W, C)), np.zeros((H, W, C))
    bG, _ = begin(lv.live, fixed, G)
    bs = [ch.rhs(lv, None if gx is None else gx[..., c], None if gy is None else gy[..., c], fa[..., c], va[..., c]) for c in range(C)]
    epsilon = epsilon_rel * float(np.sqrt(sum(np.sum(b * b) for b in bs)))
    for c in range(C):
        x0 = ch.x_after(lv, np.zeros((H, W)), fa[..., c], va[..., c], init=True)
        u[..., c], _, ok, _ = ch.pcg(levels, bs[c], epsilon, max_iteration, 2, x0, kind)
        assert ok, "the model's forward solve did not converge"
        v[..., c], _, ok, _ = ch.pcg(levels, bG[..., c], epsilon, max_iteration, 2, None, kind)
        assert ok, "the model's adjoint solve did not converge"
    return u, v, gradients(v, u, grad, gx, gy, f, wx, wy, lam, fixed), epsilon
