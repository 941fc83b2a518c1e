"""Test-side expectations of the line smoother of weighted grid handles (include/ccp_gs.h, CCP_MG_SMOOTHER_LINE), NOT
product code.

A numpy model of csrc/ccp_grid_mgl.hpp's V-cycle on the hierarchies of weighted_helpers / rescaled_helpers /
constrained_helpers (which this file imports):

* the levels above the tail (level 0, and every level with a side > 32) smooth by alternating zebra line relaxation:
  one sweep = x-lines of even rows, x-lines of odd rows, y-lines of even columns, y-lines of odd columns; every line
  is solved exactly (serial Thomas, no pivoting) with the other direction's neighbours on the right-hand side:
  rhs = b; rhs += w0 z0; rhs += w1 z1 (north then south for a row, west then east for a column);
* a dead cell (d = 0) is the identity row with right-hand side 0: z = 0 there, nothing divides by it;
* pre-smoothing: nu sweeps from z = 0; post-smoothing: z += cs * e_c on live pixels, then nu sweeps in the reverse
  order (y odd, y even, x odd, x even);
* the tail levels (the first level below level 0 whose sides are both <= 32, and everything below it) run red-black
  exactly as mg_helpers.vcycle; cs is 2.0 on a Galerkin hierarchy and 1.0 on a rescaled one.

The device solves a line with a partitioned elimination and cyclic reduction, so its bits differ from Thomas's: the
device is compared with a tolerance, taken from the deviation of this model in float64 from the same model carried in
np.longdouble (`deviation`).  Every function works in the dtype of the arrays it is given."""
import math

import numpy as np

import mg_helpers as mg

TAIL_SIDE = 32
CS = {"galerkin": 2.0, "rescaled": 1.0}


def tail_level(levels):
    """The first level of the tail (>= 1): lines on the levels before it."""
    for k in range(1, len(levels)):
        if levels[k].W <= TAIL_SIDE and levels[k].H <= TAIL_SIDE:
            return k
    return len(levels)


def thomas(lo, d, up, rhs):
    """Solve lo[i] x[i-1] + d[i] x[i] + up[i] x[i+1] = rhs[i] along axis 0 (all lines of axis 1 at once)."""
    n = d.shape[0]
    cp = np.zeros_like(d)
    y = np.zeros_like(d)
    cp[0] = up[0] / d[0]
    y[0] = rhs[0] / d[0]
    for i in range(1, n):
        den = d[i] - lo[i] * cp[i - 1]
        cp[i] = up[i] / den
        y[i] = (rhs[i] - lo[i] * y[i - 1]) / den
    x = np.zeros_like(d)
    x[n - 1] = y[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = y[i] - cp[i] * x[i + 1]
    return x


def _solve_lines(d, w, rhs):
    """Lines along axis 0: diagonal d, w[i] the weight between i and i + 1 (w[n-1] unused), right-hand side rhs."""
    dead = d == 0
    zero = np.zeros_like(d)
    wl = np.where(dead, zero, w)
    wl[-1] = 0
    up = -wl
    lo = zero.copy()
    lo[1:] = np.where(dead[1:], zero[1:], -wl[:-1])
    one = np.ones_like(d)
    return thomas(lo, np.where(dead, one, d), up, np.where(dead, zero, rhs))


def x_lines(lv, z, b, parity, first=False):
    """The rows of parity `parity`, in place."""
    rows = slice(parity, lv.H, 2)
    rhs = b[rows].copy()
    if not first:
        zn, zs = mg._shift(z, -1, 0), mg._shift(z, 1, 0)
        rhs = rhs + mg._shift(lv.ws, -1, 0)[rows] * zn[rows]
        rhs = rhs + lv.ws[rows] * zs[rows]
    if rhs.shape[0]:
        z[rows] = _solve_lines(lv.d[rows].T.copy(), lv.we[rows].T.copy(), rhs.T.copy()).T


def y_lines(lv, z, b, parity):
    """The columns of parity `parity`, in place."""
    cols = slice(parity, lv.W, 2)
    zw, ze = mg._shift(z, 0, -1), mg._shift(z, 0, 1)
    rhs = b[:, cols].copy()
    rhs = rhs + mg._shift(lv.we, 0, -1)[:, cols] * zw[:, cols]
    rhs = rhs + lv.we[:, cols] * ze[:, cols]
    if rhs.shape[1]:
        z[:, cols] = _solve_lines(lv.d[:, cols].copy(), lv.ws[:, cols].copy(), rhs)


def cast(levels, dtype):
    """The same operators (the same bits) carried in `dtype`."""
    return [mg.Coarse(lv.d.astype(dtype), lv.we.astype(dtype), lv.ws.astype(dtype)) for lv in levels]


def vcycle(levels, b, nu=1, cs=1.0, k=0, tail=None):
    """z = M^-1 b on level k."""
    tail = tail_level(levels) if tail is None else tail
    lv = levels[k]
    z = np.zeros_like(b)
    if k == len(levels) - 1:
        if k == 0:
            lv.sweep(z, b, mg.RED, first=True)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(lv.live, b / lv.d, np.zeros_like(b))
        return z
    lines = k < tail
    for s in range(nu):
        if lines:
            x_lines(lv, z, b, 0, first=(s == 0))
            x_lines(lv, z, b, 1)
            y_lines(lv, z, b, 0)
            y_lines(lv, z, b, 1)
        else:
            lv.sweep(z, b, mg.RED, first=(s == 0))
            lv.sweep(z, b, mg.BLACK)
    e = vcycle(levels, mg.restrict(lv.residual(z, b)), nu, cs, k + 1, tail)
    up = np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)[:lv.H, :lv.W]
    z = np.where(lv.live, z + b.dtype.type(cs) * up, z)
    for _ in range(nu):
        if lines:
            y_lines(lv, z, b, 1)
            y_lines(lv, z, b, 0)
            x_lines(lv, z, b, 1)
            x_lines(lv, z, b, 0)
        else:
            lv.sweep(z, b, mg.BLACK)
            lv.sweep(z, b, mg.RED)
    return z


def deviation(levels, b, nu=1, cs=1.0):
    """(max |z64 - z80| / max |z80|, z64): one V-cycle of the float64 model against the np.longdouble model."""
    z64 = vcycle(cast(levels, np.float64), np.asarray(b, dtype=np.float64), nu, cs)
    z80 = vcycle(cast(levels, np.longdouble), np.asarray(b, dtype=np.longdouble), nu, cs)
    return float(np.max(np.abs(z64 - z80)) / np.max(np.abs(z80))), z64


def pcg(levels, b, epsilon, max_iteration, nu=1, cs=1.0, x0=None, precondition=None):
    """mg_helpers.pcg with the line V-cycle (or with `precondition`, a function r -> z): (x, iterations, converged,
    last sqrt(r'r)).  levels[0] needs `apply` (a weighted level 0)."""
    A = levels[0]
    M = precondition if precondition is not None else (lambda r: vcycle(levels, r, nu, cs))
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A.apply(x)
    rr = float(np.sum(r * r))
    if math.sqrt(rr) < epsilon:
        return x, 0, True, math.sqrt(rr)
    z = M(r)
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
        z = M(r)
        rz_new = float(np.sum(r * z))
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        cnt += 1
    return x, cnt, False, norm


def preconditioner_matrix(levels, nu=1, cs=1.0):
    """M^-1 as a dense matrix on the live pixels of level 0 (one V-cycle per unit vector), and the live indices."""
    lv = levels[0]
    live = np.flatnonzero(lv.live.ravel())
    M = np.zeros((len(live), len(live)))
    for j, i in enumerate(live):
        e = np.zeros(lv.W * lv.H)
        e[i] = 1.0
        M[:, j] = vcycle(levels, e.reshape(lv.H, lv.W), nu, cs).ravel()[live]
    return M, live


# ---- the systems of the tests ---------------------------------------------------------------------------------------
def image(W, H, seed=7):
    """tools/weighted_bench.py's image in numpy: flat 16-px patches x 230 plus 25 x noise, one channel, u8."""
    rng = np.random.default_rng(seed)
    patches = rng.random((H // 16 + 1, W // 16 + 1))
    img = np.repeat(np.repeat(patches, 16, axis=0), 16, axis=1)[:H, :W] * 230.0
    return np.clip(img + 25.0 * rng.random((H, W)), 0, 255).astype(np.uint8)


def wls_weights(img, lam=1.0, alpha=1.2, eps=1e-4):
    """tensor_ops.wls_weights in numpy, as the float32 H x W arrays a handle takes (the last column of wx and the
    last row of wy are 0)."""
    lum = img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)
    ell = np.log(lum + eps)
    wx = np.zeros_like(ell)
    wy = np.zeros_like(ell)
    wx[:, :-1] = lam / (np.abs(ell[:, 1:] - ell[:, :-1]) ** alpha + eps)
    wy[:-1, :] = lam / (np.abs(ell[1:, :] - ell[:-1, :]) ** alpha + eps)
    return wx.astype(np.float32), wy.astype(np.float32)


def anchors(W, H, step):
    """Fixed pixels at [8::step, 8::step]."""
    fixed = np.zeros((H, W), dtype=np.uint8)
    fixed[8::step, 8::step] = 1
    return fixed


def wls_system(W, H, kind="rescaled"):
    """(levels, b) of WLS smoothing of image(W, H): lambda = 1, b = lambda f."""
    import rescaled_helpers as rh
    import weighted_helpers as wh
    img = image(W, H)
    wx, wy = wls_weights(img)
    lam = np.ones((H, W), dtype=np.float32)
    levels = (rh if kind == "rescaled" else wh).hierarchy(W, H, wx, wy, lam)
    return levels, levels[0].lam * img.astype(np.float64)


def anchor_system(W, H, step, kind="rescaled"):
    """(levels, b, fixed) of sparse-anchor interpolation: the WLS weights of image(W, H), lambda = 0, the pixels
    [8::step, 8::step] fixed at the image's values."""
    import constrained_helpers as ch
    img = image(W, H)
    wx, wy = wls_weights(img)
    fixed = anchors(W, H, step)
    levels = ch.hierarchy(W, H, wx, wy, None, fixed, kind)
    return levels, ch.rhs(levels[0], values=img), fixed


def shape_fixed(W, H):
    """Fixed pixels that split lines every way: the outside of an ellipse, one whole row, one whole column, and
    isolated pixels inside lines (also two apart: a segment of length 1 between them)."""
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = (((xx - W / 2.0) / (0.46 * W)) ** 2 + ((yy - H / 2.0) / (0.44 * H)) ** 2 > 1.0).astype(np.uint8)
    fixed[H // 3, :] = 1
    fixed[:, W // 4] = 1
    for x, y in ((W // 2, H // 2), (W // 2 + 2, H // 2), (W // 2, H // 2 + 5), (W // 2, H // 2 + 7), (W // 2 + 9, H // 2 + 20),
                 (W // 2 + 31, H // 2 - 11)):
        fixed[y, x] = 1
    return fixed


def shape_system(W, H, kind, fixed=False, seed=5):
    """(levels, b, wx, wy, lam, fixed or None) of a V-cycle test shape: WLS weights of image(W, H), lambda = 1, and a
    seeded right-hand side (0 on fixed pixels)."""
    import constrained_helpers as ch
    img = image(W, H)
    wx, wy = wls_weights(img)
    lam = np.ones((H, W), dtype=np.float32)
    fx = shape_fixed(W, H) if fixed else None
    levels = ch.hierarchy(W, H, wx, wy, lam, fx, kind)
    b = np.random.default_rng(seed).normal(size=(H, W)) * 100.0
    return levels, np.where(levels[0].live, b, 0.0), wx, wy, lam, fx
