"""Test-side expectations of the multigrid-preconditioned CG (ccp_grid_mg_*), NOT product code.

A numpy restatement of csrc/ccp_grid_mg.hpp in the same operation order, so that the device's hierarchy and V-cycle
can be compared bit for bit:

* level 0 is SolveChannel's matrix (`classify`) or the Dirichlet-mask Laplacian; a pixel is dead if its diagonal is 0;
* level k+1 is ceil(W_k/2) x ceil(H_k/2), coarse cell (X,Y) aggregates the live pixels of (2X..2X+1, 2Y..2Y+1), and
  A_{k+1} = P^T A_k P is stored as (d, we, ws): diagonal and the positive weights to the east and south cells;
* V-cycle: nu red-black sweeps (red, black) from z = 0, residual restricted as (r00 + r10) + (r01 + r11), recursion,
  z += 2.0 * e_c on live pixels, nu sweeps (black, red); the 1x1 level solves z = b/d;
* level-0 sweeps and residuals are gs_update / apply_row (or the masked kernels' interior formula); coarse levels use
  s = 0; s += wN xN; s += wW xW; s += wE xE; s += wS xS; x = (b + s) / d and r = b - (d x - s).

Arrays are H x W in raster order.  `pcg` is the loop of ccp_grid_mg_conjugate_gradient with numpy's dot products (the
device's are tree-ordered: iteration counts agree to +-1, iterates to rounding)."""
import math

import numpy as np

RED, BLACK = 0, 1


def _shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx], 0.0 outside."""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def colour(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx + yy) & 1


class Level0:
    """The handle's operator: SolveChannel's matrix (mask None) or the Dirichlet-mask Laplacian."""

    def __init__(self, W, H, mask=None):
        self.W, self.H = W, H
        yy, xx = np.mgrid[0:H, 0:W]
        if mask is None:
            self.mask = None
            here = (xx < W - 1) & (yy < H - 1)
            self.up = (yy >= 1) & (xx < W - 1)
            self.left = (xx >= 1) & (yy < H - 1)
            self.right = here
            self.down = here
            self.diag = (self.up.astype(np.int64) + self.left + 2 * here + ((xx | yy) == 0)).astype(np.float64)
        else:
            m = np.asarray(mask) != 0
            assert m.shape == (H, W)
            self.mask = m
            self.diag = np.where(m, 4.0, 0.0)
        self.live = self.diag != 0

    def coefficients(self):
        """(d, we, ws) of level 0."""
        if self.mask is None:
            return self.diag.copy(), self.right.astype(np.float64), self.down.astype(np.float64)
        m = self.mask
        we = (m & _shift(m.astype(np.int64), 0, 1).astype(bool)).astype(np.float64)
        ws = (m & _shift(m.astype(np.int64), 1, 0).astype(bool)).astype(np.float64)
        return self.diag.copy(), we, ws

    def sweep(self, z, b, c, first=False):
        """Half-sweep of colour c in place; dead pixels of the colour are written 0."""
        zn = np.zeros_like(z) if first else z
        xu, xl, xr, xd = _shift(zn, -1, 0), _shift(zn, 0, -1), _shift(zn, 0, 1), _shift(zn, 1, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.mask is None:                                   # gs_update
                sigma = np.zeros_like(z)
                sigma = np.where(self.up, sigma + (-1.0 * xu), sigma)
                sigma = np.where(self.left, sigma + (-1.0 * xl), sigma)
                sigma = np.where(self.right, sigma + (-1.0 * xr), sigma)
                sigma = np.where(self.down, sigma + (-1.0 * xd), sigma)
                new = np.where(self.live, (b - sigma) / self.diag, 0.0)
            else:                                                   # the masked kernels' interior formula
                new = np.where(self.mask, (b + (((xu + xl) + xr) + xd)) * 0.25, 0.0)
        sel = colour(self.H, self.W) == c
        z[sel] = new[sel]

    def apply(self, z):
        """A z in applyToVector's order (apply_row / k_apply's masked row); 0 on dead pixels."""
        xu, xl, xr, xd = _shift(z, -1, 0), _shift(z, 0, -1), _shift(z, 0, 1), _shift(z, 1, 0)
        s = np.zeros_like(z)
        if self.mask is None:
            s = np.where(self.up, s + (-1.0 * xu), s)
            s = np.where(self.left, s + (-1.0 * xl), s)
            s = np.where(self.live, s + self.diag * z, s)
            s = np.where(self.right, s + (-1.0 * xr), s)
            s = np.where(self.down, s + (-1.0 * xd), s)
            return s
        s = s + (-1.0 * xu)
        s = s + (-1.0 * xl)
        s = s + 4.0 * z
        s = s + (-1.0 * xr)
        s = s + (-1.0 * xd)
        return np.where(self.mask, s, 0.0)

    def residual(self, z, b):
        return np.where(self.live, b - self.apply(z), 0.0)


class Coarse:
    """A coarse level: (d, we, ws)."""

    def __init__(self, d, we, ws):
        self.d, self.we, self.ws = d, we, ws
        self.H, self.W = d.shape
        self.live = d != 0

    def coefficients(self):
        return self.d, self.we, self.ws

    def _s(self, z):
        s = np.zeros_like(z)
        s = s + _shift(self.ws, -1, 0) * _shift(z, -1, 0)
        s = s + _shift(self.we, 0, -1) * _shift(z, 0, -1)
        s = s + self.we * _shift(z, 0, 1)
        s = s + self.ws * _shift(z, 1, 0)
        return s

    def sweep(self, z, b, c, first=False):
        s = self._s(np.zeros_like(z) if first else z)
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(self.live, (b + s) / self.d, 0.0)
        sel = colour(self.H, self.W) == c
        z[sel] = new[sel]

    def residual(self, z, b):
        return np.where(self.live, b - (self.d * z - self._s(z)), 0.0)


def _pad_even(a):
    H, W = a.shape
    out = np.zeros((H + (H & 1), W + (W & 1)), dtype=a.dtype)
    out[:H, :W] = a
    return out


def coarsen(level):
    d, we, ws = (_pad_even(a) for a in level.coefficients())
    dc = ((d[0::2, 0::2] + d[0::2, 1::2]) + (d[1::2, 0::2] + d[1::2, 1::2])) \
        - 2.0 * ((we[0::2, 0::2] + we[1::2, 0::2]) + (ws[0::2, 0::2] + ws[0::2, 1::2]))
    wec = we[0::2, 1::2] + we[1::2, 1::2]
    wsc = ws[1::2, 0::2] + ws[1::2, 1::2]
    return Coarse(dc, wec, wsc)


def hierarchy(W, H, mask=None):
    levels = [Level0(W, H, mask)]
    while levels[-1].W > 1 or levels[-1].H > 1:
        levels.append(coarsen(levels[-1]))
    return levels


def restrict(r):
    r = _pad_even(r)
    return (r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2])


def vcycle(levels, b, nu=2, k=0):
    """z = M^-1 b on level k."""
    lv = levels[k]
    z = np.zeros_like(b)
    if k == len(levels) - 1:
        if k == 0:
            lv.sweep(z, b, RED, first=True)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(lv.live, b / lv.d, 0.0)
        return z
    for s in range(nu):
        lv.sweep(z, b, RED, first=(s == 0))
        lv.sweep(z, b, BLACK)
    e = vcycle(levels, restrict(lv.residual(z, b)), nu, k + 1)
    up = np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)[:lv.H, :lv.W]
    z = np.where(lv.live, z + 2.0 * up, z)
    for _ in range(nu):
        lv.sweep(z, b, BLACK)
        lv.sweep(z, b, RED)
    return z


def pcg(levels, b, epsilon, max_iteration, nu=2, x0=None):
    """(x, iterations, converged, last sqrt(r'r)) of ccp_grid_mg_conjugate_gradient on one channel (H x W arrays)."""
    A = levels[0]
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A.apply(x)
    rr = float(np.sum(r * r))
    if math.sqrt(rr) < epsilon:
        return x, 0, True, math.sqrt(rr)
    z = vcycle(levels, r, nu)
    rz = float(np.sum(r * z))
    p = z.copy()
    cnt = 0
    norm = math.sqrt(rr)
    while cnt < max_iteration:
        ap = A.apply(p)
        alpha = rz / float(np.sum(p * ap))
        x = x + alpha * p
        r = r + (-alpha) * ap
        norm = math.sqrt(float(np.sum(r * r)))
        if norm < epsilon:
            return x, cnt, True, norm
        z = vcycle(levels, r, nu)
        rz_new = float(np.sum(r * z))
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        cnt += 1
    return x, cnt, False, norm
