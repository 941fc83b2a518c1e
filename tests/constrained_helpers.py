"""Test-side expectations of weighted grid handles with fixed pixels (include/ccp_gs.h, "Hard constraints on weighted
grids"), NOT product code.

A numpy restatement of the header's formulas in the device's operation order, on top of weighted_helpers /
rescaled_helpers (whose coarsening, V-cycle and PCG run unchanged on the level 0 built here):

* free pixel: d = lam; += wN; += wW; += wE; += wS over all in-canvas edges (weighted_helpers.coefficients, unchanged);
  stored we / ws = the weight where both ends are free, else 0; lam' = lam; += cN; += cW; += cE; += cS over the fixed
  neighbours (free neighbours skipped);
* fixed pixel: d = we = ws = lam' = 0;
* ce / cs: the east / south edge's weight where exactly one end is fixed, else 0;
* b of a free pixel: t = 0; += wN gy(x,y-1); += wW gx(x-1,y); += -(wE gx); += -(wS gy); += lam f with the ORIGINAL
  weights and the caller's lam, then += cN v(x,y-1); += cW v(x-1,y); += cE v(x+1,y); += cS v(x,y+1) over the fixed
  neighbours; b = 0 on fixed pixels;
* x after the assembly: v on fixed pixels; with init f on live free pixels and 0 on dead free ones, else unchanged.
"""
import numpy as np

import rescaled_helpers as rh
import weighted_helpers as wh


class Level0(wh.Level0):
    """Level 0 of a constrained operator: `lam` is lam' (what the coarsening carries); lam0, ce, cs and fixed are what
    the right-hand side needs."""

    def __init__(self, d, we, ws, lam_mg, lam0, ce, cs, fixed):
        super().__init__(d, we, ws, lam_mg)
        self.lam0, self.ce, self.cs, self.fixed = lam0, ce, cs, fixed


def _shift_mask(m, dy, dx):
    """m at (y + dy, x + dx), False outside the canvas."""
    H, W = m.shape
    out = np.zeros_like(m)
    ys = slice(max(0, -dy), H - max(0, dy))
    xs = slice(max(0, -dx), W - max(0, dx))
    yt = slice(max(0, dy), H - max(0, -dy))
    xt = slice(max(0, dx), W - max(0, -dx))
    out[ys, xs] = m[yt, xt]
    return out


def _shift(a, dy, dx):
    """a at (y + dy, x + dx), 0 outside the canvas."""
    H, W = a.shape
    out = np.zeros_like(a)
    ys = slice(max(0, -dy), H - max(0, dy))
    xs = slice(max(0, -dx), W - max(0, dx))
    yt = slice(max(0, dy), H - max(0, -dy))
    xt = slice(max(0, dx), W - max(0, -dx))
    out[ys, xs] = a[yt, xt]
    return out


def level0(W, H, wx=None, wy=None, lam=None, fixed=None):
    d, we, ws, lam0 = wh.coefficients(W, H, wx, wy, lam)
    fx = np.zeros((H, W), bool) if fixed is None else (np.asarray(fixed) != 0)
    fN, fW, fE, fS = _shift_mask(fx, -1, 0), _shift_mask(fx, 0, -1), _shift_mask(fx, 0, 1), _shift_mask(fx, 1, 0)
    wN, wW = _shift(ws, -1, 0), _shift(we, 0, -1)
    lp = lam0.copy()
    lp = np.where(fN, lp + wN, lp)
    lp = np.where(fW, lp + wW, lp)
    lp = np.where(fE, lp + we, lp)
    lp = np.where(fS, lp + ws, lp)
    east_exists = np.zeros((H, W), bool)
    east_exists[:, :W - 1] = True
    south_exists = np.zeros((H, W), bool)
    south_exists[:H - 1, :] = True
    be = east_exists & (fx != fE)
    bs = south_exists & (fx != fS)
    return Level0(np.where(fx, 0.0, d), np.where(fx | fE, 0.0, we), np.where(fx | fS, 0.0, ws), np.where(fx, 0.0, lp), lam0,
                  np.where(be, we, 0.0), np.where(bs, ws, 0.0), fx)


def hierarchy(W, H, wx=None, wy=None, lam=None, fixed=None, kind="galerkin"):
    coarsen = rh.coarsen if kind == "rescaled" else wh.coarsen
    levels = [level0(W, H, wx, wy, lam, fixed)]
    while levels[-1].W > 1 or levels[-1].H > 1:
        levels.append(coarsen(levels[-1]))
    return levels


def vcycle(levels, b, nu=2, kind="galerkin"):
    return rh.vcycle(levels, b, nu) if kind == "rescaled" else wh.vcycle(levels, b, nu)


def pcg(levels, b, epsilon, max_iteration, nu=2, x0=None, kind="galerkin"):
    return (rh.pcg if kind == "rescaled" else wh.pcg)(levels, b, epsilon, max_iteration, nu, x0)


def rhs(lv, gx=None, gy=None, f=None, values=None):
    """b of one channel (H x W): float32 guidance, data and prescribed values of any dtype (None: 0)."""
    H, W = lv.d.shape
    z = np.zeros((H, W))
    gx = z if gx is None else np.asarray(gx, dtype=np.float32).astype(np.float64)
    gy = z if gy is None else np.asarray(gy, dtype=np.float32).astype(np.float64)
    f = z if f is None else np.asarray(f).astype(np.float64)
    v = z if values is None else np.asarray(values).astype(np.float64)
    we, ws = lv.we + lv.ce, lv.ws + lv.cs                      # the original weights: one of the two is 0
    t = np.zeros((H, W))
    t[1:, :] = t[1:, :] + ws[:-1, :] * gy[:-1, :]
    t[:, 1:] = t[:, 1:] + we[:, :-1] * gx[:, :-1]
    t[:, :W - 1] = t[:, :W - 1] + (-(we[:, :W - 1] * gx[:, :W - 1]))
    t[:H - 1, :] = t[:H - 1, :] + (-(ws[:H - 1, :] * gy[:H - 1, :]))
    t = t + lv.lam0 * f
    fx = lv.fixed
    with np.errstate(invalid="ignore"):
        t = np.where(_shift_mask(fx, -1, 0), t + _shift(ws, -1, 0) * _shift(v, -1, 0), t)
        t = np.where(_shift_mask(fx, 0, -1), t + _shift(we, 0, -1) * _shift(v, 0, -1), t)
        t = np.where(_shift_mask(fx, 0, 1), t + we * _shift(v, 0, 1), t)
        t = np.where(_shift_mask(fx, 1, 0), t + ws * _shift(v, 1, 0), t)
    return np.where(fx, 0.0, t)


def x_after(lv, x_before, f=None, values=None, init=False):
    """x of one channel after the assembly call."""
    H, W = lv.d.shape
    v = np.zeros((H, W)) if values is None else np.asarray(values).astype(np.float64)
    x = np.array(x_before, dtype=np.float64)
    if init:
        fv = np.zeros((H, W)) if f is None else np.asarray(f).astype(np.float64)
        x = np.where(lv.live, fv, 0.0)
    return np.where(lv.fixed, v, x)


def counts(lv):
    """(fixed pixels, free live pixels, edges with exactly one fixed end): ccp_grid_constraint_info."""
    fx = lv.fixed
    edges = int((fx[:, 1:] != fx[:, :-1]).sum() + (fx[1:, :] != fx[:-1, :]).sum())
    return int(fx.sum()), int((~fx & (lv.d != 0)).sum()), edges


# ---- scipy forms -------------------------------------------------------------------------------------------------------
def free_system(W, H, wx, wy, lam, fixed, gx=None, gy=None, f=None, values=None):
    """(A_ff, b_f, free indices): the unconstrained operator and b of weighted_helpers with the fixed pixels substituted --
    the derivative of the energy over the free pixels."""
    full = wh.Level0(*wh.coefficients(W, H, wx, wy, lam))
    A = wh.matrix(full).tocsr()
    b = wh.rhs(full, gx, gy, f).ravel()
    fx = (np.asarray(fixed) != 0).ravel()
    free, fix = np.flatnonzero(~fx), np.flatnonzero(fx)
    v = np.zeros(W * H) if values is None else np.asarray(values, dtype=np.float64).ravel()
    return A[free][:, free], b[free] - A[free][:, fix] @ v[fix], free
