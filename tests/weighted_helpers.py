"""Test-side expectations of the weighted grid handles (include/ccp_gs.h, CCP_GRID_WEIGHTED), NOT product code.

A numpy restatement of csrc/ccp_grid_weighted.hpp and of the weighted hierarchy of csrc/ccp_grid_mg.hpp in the device's
operation order, so that the operator, b, the product, the hierarchy and one V-cycle compare bit for bit:

* weights are float32 H x W arrays (or None: wx = wy = 1, lam = 0) widened to float64;
* d = lam; d += wN; d += wW; d += wE; d += wS (edges outside the canvas skipped); we = wx, ws = wy where the edge
  exists, else 0;
* b = 0; += wN gy(x,y-1); += wW gx(x-1,y); += -(wE gx); += -(wS gy); += lam f;
* A z = 0; += -(wN zN); += -(wW zW); += d z; += -(wE zE); += -(wS zS), 0 on dead pixels;
* coarsening: lam_c = (l00 + l10) + (l01 + l11); d_c = lam_c; += north; += west; += east; += south;
* the V-cycle is mg_helpers.vcycle with level 0 a stored operator (mg_helpers.Coarse: its sweeps and residual).
"""
import numpy as np

import mg_helpers as mg


def _f64(a, H, W, default):
    if a is None:
        return np.full((H, W), default, dtype=np.float64)
    return np.asarray(a, dtype=np.float32).astype(np.float64) if np.asarray(a).dtype != np.float64 else np.asarray(a, dtype=np.float64)


def coefficients(W, H, wx=None, wy=None, lam=None):
    """(d, we, ws, lam) of level 0, float64 H x W."""
    wx, wy, lam = _f64(wx, H, W, 1.0), _f64(wy, H, W, 1.0), _f64(lam, H, W, 0.0)
    we = np.zeros((H, W))
    ws = np.zeros((H, W))
    we[:, :W - 1] = wx[:, :W - 1]
    ws[:H - 1, :] = wy[:H - 1, :]
    d = lam.copy()
    d[1:, :] = d[1:, :] + ws[:-1, :]            # wN
    d[:, 1:] = d[:, 1:] + we[:, :-1]            # wW
    d[:, :W - 1] = d[:, :W - 1] + we[:, :W - 1]  # wE
    d[:H - 1, :] = d[:H - 1, :] + ws[:H - 1, :]  # wS
    return d, we, ws, lam.copy()


def solve_channel_weights(W, H):
    """SolveChannel's matrix as weights: wx = wy = 1 on x < W-1 and y < H-1, lam = 1 at (0,0)."""
    yy, xx = np.mgrid[0:H, 0:W]
    cell = ((xx < W - 1) & (yy < H - 1)).astype(np.float32)
    lam = np.zeros((H, W), dtype=np.float32)
    lam[0, 0] = 1.0
    return cell, cell.copy(), lam


def rhs(level, gx=None, gy=None, f=None):
    """b of one channel (H x W) from float32 H x W guidance / data (None: 0)."""
    H, W = level.d.shape
    z = np.zeros((H, W))
    gx = z if gx is None else np.asarray(gx, dtype=np.float32).astype(np.float64)
    gy = z if gy is None else np.asarray(gy, dtype=np.float32).astype(np.float64)
    f = z if f is None else np.asarray(f).astype(np.float64)
    t = np.zeros((H, W))
    t[1:, :] = t[1:, :] + level.ws[:-1, :] * gy[:-1, :]
    t[:, 1:] = t[:, 1:] + level.we[:, :-1] * gx[:, :-1]
    t[:, :W - 1] = t[:, :W - 1] + (-(level.we[:, :W - 1] * gx[:, :W - 1]))
    t[:H - 1, :] = t[:H - 1, :] + (-(level.ws[:H - 1, :] * gy[:H - 1, :]))
    return t + level.lam * f


class Level0(mg.Coarse):
    """A weighted handle's level 0: a stored operator (the coarse levels' sweeps and residual) with lam and the PCG's
    product."""

    def __init__(self, d, we, ws, lam):
        super().__init__(d, we, ws)
        self.lam = lam

    def apply(self, z):
        s = np.zeros_like(z)
        s = s + (-(mg._shift(self.ws, -1, 0) * mg._shift(z, -1, 0)))
        s = s + (-(mg._shift(self.we, 0, -1) * mg._shift(z, 0, -1)))
        s = s + self.d * z
        s = s + (-(self.we * mg._shift(z, 0, 1)))
        s = s + (-(self.ws * mg._shift(z, 1, 0)))
        return np.where(self.live, s, 0.0)


class Coarse(mg.Coarse):
    def __init__(self, d, we, ws, lam):
        super().__init__(d, we, ws)
        self.lam = lam


def coarsen(level):
    """The cancellation-free Galerkin coarsening (k_weighted_coarsen)."""
    H, W = level.d.shape
    lam, we, ws = (mg._pad_even(a) for a in (level.lam, level.we, level.ws))
    # one more row / column of zeros above and to the left: the edges that enter an aggregate from the north / west
    wsp = np.zeros((lam.shape[0] + 1, lam.shape[1]))
    wsp[1:, :] = ws
    wep = np.zeros((lam.shape[0], lam.shape[1] + 1))
    wep[:, 1:] = we
    lc = (lam[0::2, 0::2] + lam[0::2, 1::2]) + (lam[1::2, 0::2] + lam[1::2, 1::2])
    north = wsp[0:-1:2, 0::2] + wsp[0:-1:2, 1::2]
    west = wep[0::2, 0:-1:2] + wep[1::2, 0:-1:2]
    east = we[0::2, 1::2] + we[1::2, 1::2]
    south = ws[1::2, 0::2] + ws[1::2, 1::2]
    d = lc.copy()
    d = d + north
    d = d + west
    d = d + east
    d = d + south
    return Coarse(d, east, south, lc)


def hierarchy(W, H, wx=None, wy=None, lam=None):
    levels = [Level0(*coefficients(W, H, wx, wy, lam))]
    while levels[-1].W > 1 or levels[-1].H > 1:
        levels.append(coarsen(levels[-1]))
    return levels


def vcycle(levels, b, nu=2):
    return mg.vcycle(levels, b, nu)


def pcg(levels, b, epsilon, max_iteration, nu=2, x0=None):
    return mg.pcg(levels, b, epsilon, max_iteration, nu, x0)


# ---- scipy forms (the checks of tests/test_weighted_helpers.py) --------------------------------------------------------
def difference_matrices(W, H):
    """Dx (rows: the edges (x,y)-(x+1,y), x < W-1) and Dy (rows: (x,y)-(x,y+1), y < H-1) on raster-ordered pixels."""
    import scipy.sparse as sp
    idx = np.arange(W * H).reshape(H, W)
    ex = idx[:, :-1].ravel(), idx[:, 1:].ravel()
    ey = idx[:-1, :].ravel(), idx[1:, :].ravel()

    def diff(a, b):
        n = len(a)
        rows = np.concatenate([np.arange(n), np.arange(n)])
        return sp.csr_matrix((np.concatenate([-np.ones(n), np.ones(n)]), (rows, np.concatenate([a, b]))), shape=(n, W * H))
    return diff(*ex), diff(*ey)


def matrix(level):
    """The stored 5-point operator as a scipy matrix over raster-ordered pixels."""
    import scipy.sparse as sp
    H, W = level.d.shape
    idx = np.arange(W * H).reshape(H, W)
    rows = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    cols = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    vals = [level.d.ravel(), -level.we[:, :-1].ravel(), -level.we[:, :-1].ravel(), -level.ws[:-1, :].ravel(), -level.ws[:-1, :].ravel()]
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(W * H, W * H))


def preconditioner_matrix(levels, nu=2):
    """M^-1 as a dense matrix on the live pixels of level 0 (one V-cycle per unit vector), and the live indices."""
    lv = levels[0]
    live = np.flatnonzero(lv.live.ravel())
    M = np.zeros((len(live), len(live)))
    for j, i in enumerate(live):
        e = np.zeros(lv.W * lv.H)
        e[i] = 1.0
        M[:, j] = vcycle(levels, e.reshape(lv.H, lv.W), nu).ravel()[live]
    return M, live
