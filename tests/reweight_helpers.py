"""The numpy model of ccp_grid_reweight_device (include/ccp_gs.h, "Reweighting a weighted operator from the solution"):
the weights in exactly the header's operation order, the penalties psi and the energy E that an IRLS loop on them
minimises, and a dense IRLS (np.linalg.solve) for tiny canvases.

Every array operation below is element-wise fp64, one correctly rounded operation per numpy call, and the channels are
accumulated by a python loop in channel order: nothing is reassociated, so `weights` gives the bits the scalar loop
`weights_scalar` gives (tests/test_reweight_helpers.py) and the bits the kernel must give (tests/test_gpu_reweight.py)."""
import math

import numpy as np

PENALTIES = ("charbonnier", "huber", "reciprocal")
COUPLINGS = ("edge", "pixel")
PAIRS = [(p, c) for p in PENALTIES for c in COUPLINGS]


def phi(q, penalty, eps):
    eps = np.float64(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        if penalty == "charbonnier":
            return 1.0 / np.sqrt(q + eps * eps)
        if penalty == "huber":
            return 1.0 / np.fmax(np.sqrt(q), eps)
        if penalty == "reciprocal":
            return 1.0 / (np.sqrt(q) + eps)
    raise ValueError(penalty)


def _wide(a, shape=None):
    """an input widened exactly to float64 (None stays None); an H x W array serves every channel of `shape`"""
    if a is None:
        return None
    a = np.asarray(a).astype(np.float64)
    if shape is not None and a.ndim == 2:
        a = np.broadcast_to(a[:, :, None], shape)
    return a


def residuals(u, gx, gy, per_channel):
    """(q_x, q_y): H x W x sets, sets = 1 for the shared operator (all channels summed) and C for one per channel; an
    absent edge has q = +0.0"""
    u = _wide(u)
    H, W, C = u.shape
    gx, gy = _wide(gx, u.shape), _wide(gy, u.shape)
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    qx, qy = np.zeros((H, W, len(sets))), np.zeros((H, W, len(sets)))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, chans in enumerate(sets):
            ax, ay = np.zeros((H, W - 1)), np.zeros((H - 1, W))
            for c in chans:
                g = gx[:, :-1, c] if gx is not None else np.zeros((H, W - 1))
                r = g - (u[:, 1:, c] - u[:, :-1, c])
                ax = ax + r * r
                g = gy[:-1, :, c] if gy is not None else np.zeros((H - 1, W))
                r = g - (u[1:, :, c] - u[:-1, :, c])
                ay = ay + r * r
            qx[:, :-1, k] = ax
            qy[:-1, :, k] = ay
    return qx, qy


def weights(u, gx, gy, penalty, coupling, scale, eps, base_wx=None, base_wy=None, per_channel=False):
    """(wx, wy) of the header's definition, float64: H x W for the shared operator, H x W x C for one per channel; the last
    column of wx and the last row of wy are +0.0.  u: H x W x C of any dtype (widened exactly); gx, gy: H x W x C or None;
    base_*: H x W (x C) of float32 / float64, or None."""
    qx, qy = residuals(u, gx, gy, per_channel)
    shape = qx.shape
    if coupling == "pixel":
        qx = qy = qx + qy
    elif coupling != "edge":
        raise ValueError(coupling)
    scale = np.float64(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        wx, wy = scale * phi(qx, penalty, eps), scale * phi(qy, penalty, eps)
        if base_wx is not None:
            wx = _wide(base_wx, shape) * wx
        if base_wy is not None:
            wy = _wide(base_wy, shape) * wy
    wx, wy = np.array(wx), np.array(wy)
    wx[:, -1, :] = 0.0
    wy[-1, :, :] = 0.0
    return (wx, wy) if per_channel else (wx[:, :, 0], wy[:, :, 0])


def weights_scalar(u, gx, gy, penalty, coupling, scale, eps, base_wx=None, base_wy=None, per_channel=False):
    """`weights` as a scalar triple loop over y, x and the channels, one python float operation at a time: the header's
    text, line by line"""
    u = _wide(u)
    H, W, C = u.shape
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    wx, wy = np.zeros((H, W, len(sets))), np.zeros((H, W, len(sets)))
    eps, scale = float(eps), float(scale)

    def phi1(q):
        if penalty == "charbonnier":
            return 1.0 / math.sqrt(q + eps * eps)
        if penalty == "huber":
            return 1.0 / max(math.sqrt(q), eps)
        return 1.0 / (math.sqrt(q) + eps)

    def base(b, y, x, k):
        if b is None:
            return None
        b = np.asarray(b)
        return float(b[y, x]) if b.ndim == 2 else float(b[y, x, k])

    for k, chans in enumerate(sets):
        for y in range(H):
            for x in range(W):
                qx = qy = 0.0
                if x + 1 < W:
                    acc = 0.0
                    for c in chans:
                        g = float(gx[y, x, c]) if gx is not None else 0.0
                        r = g - (float(u[y, x + 1, c]) - float(u[y, x, c]))
                        acc += r * r
                    qx = acc
                if y + 1 < H:
                    acc = 0.0
                    for c in chans:
                        g = float(gy[y, x, c]) if gy is not None else 0.0
                        r = g - (float(u[y + 1, x, c]) - float(u[y, x, c]))
                        acc += r * r
                    qy = acc
                if coupling == "pixel":
                    qx = qy = qx + qy
                if x + 1 < W:
                    t = scale * phi1(qx)
                    b = base(base_wx, y, x, k)
                    wx[y, x, k] = t if b is None else b * t
                if y + 1 < H:
                    t = scale * phi1(qy)
                    b = base(base_wy, y, x, k)
                    wy[y, x, k] = t if b is None else b * t
    return (wx, wy) if per_channel else (wx[:, :, 0], wy[:, :, 0])


def psi(rho, penalty, eps):
    """the penalty whose derivative is rho * phi(rho^2)"""
    rho = np.asarray(rho, dtype=np.float64)
    if penalty == "charbonnier":
        return np.sqrt(rho * rho + eps * eps)
    if penalty == "huber":
        return np.where(rho < eps, rho * rho / (2.0 * eps), rho - eps / 2.0)
    if penalty == "reciprocal":
        return rho - eps * np.log1p(rho / eps)
    raise ValueError(penalty)


def energy(u, gx, gy, f, penalty, coupling, strength, eps, data_weight=1.0, per_channel=False):
    """E(u) = sum 2 strength psi(rho) + sum data_weight (u - f)^2 with unit base weights: over the edges ("edge": rho the
    edge's own residual) or over the pixels ("pixel": rho^2 = q_x + q_y)"""
    u, f = _wide(u), _wide(f)
    qx, qy = residuals(u, gx, gy, per_channel)
    if coupling == "pixel":
        reg = psi(np.sqrt(qx + qy), penalty, eps).sum()
    else:
        reg = psi(np.sqrt(qx[:, :-1]), penalty, eps).sum() + psi(np.sqrt(qy[:-1]), penalty, eps).sum()
    return float(2.0 * strength * reg + (data_weight * (u - f) ** 2).sum())


def system(wx, wy, lam, gx, gy, f):
    """(A, b) of one channel: minimise sum wx (uE - u - gx)^2 + sum wy (uS - u - gy)^2 + sum lam (u - f)^2 over an H x W
    plane, dense, pixels in row-major order"""
    H, W = wx.shape
    n = H * W
    A, b = np.zeros((n, n)), np.zeros(n)
    idx = np.arange(n).reshape(H, W)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (H, W))
    A[idx.ravel(), idx.ravel()] += lam.ravel()
    b += (lam * f).ravel()
    for w, g, p, q in ((wx[:, :-1], None if gx is None else gx[:, :-1], idx[:, :-1], idx[:, 1:]),
                       (wy[:-1], None if gy is None else gy[:-1], idx[:-1], idx[1:])):
        p, q, w = p.ravel(), q.ravel(), w.ravel()
        np.add.at(A, (p, p), w)
        np.add.at(A, (q, q), w)
        np.add.at(A, (p, q), -w)
        np.add.at(A, (q, p), -w)
        if g is not None:
            np.add.at(b, q, w * g.ravel())
            np.add.at(b, p, -w * g.ravel())
    return A, b


def true_residual(u, wx, wy, lam, gx, gy, f):
    """|b - A u| and |b| per channel of the system `system` builds, matrix-free (u, f: H x W x C; wx, wy: H x W or
    H x W x C; gx, gy: H x W x C or None)"""
    u, f = _wide(u), _wide(f)
    H, W, C = u.shape
    wx, wy = _wide(wx, u.shape), _wide(wy, u.shape)
    lam = np.asarray(lam, dtype=np.float64)
    lam = np.broadcast_to(lam[:, :, None] if lam.ndim == 2 else lam, u.shape)
    ex = wx[:, :-1] * ((gx[:, :-1] if gx is not None else 0.0) - (u[:, 1:] - u[:, :-1]))
    ey = wy[:-1] * ((gy[:-1] if gy is not None else 0.0) - (u[1:] - u[:-1]))
    r = lam * (f - u)                                         # b - A u = lam (f - u) + the edges' w (g - du), signed by the end
    r[:, 1:] += ex
    r[:, :-1] -= ex
    r[1:] += ey
    r[:-1] -= ey
    gxw = wx[:, :-1] * (gx[:, :-1] if gx is not None else 0.0) + np.zeros_like(ex)
    gyw = wy[:-1] * (gy[:-1] if gy is not None else 0.0) + np.zeros_like(ey)
    b = lam * f
    b[:, 1:] += gxw
    b[:, :-1] -= gxw
    b[1:] += gyw
    b[:-1] -= gyw
    return np.sqrt((r * r).sum(axis=(0, 1))), np.sqrt((b * b).sum(axis=(0, 1)))


def dense_irls(f, gx, gy, penalty, coupling, strength, eps, data_weight, outer, per_channel=False, perturb=None, seed=0):
    """The IRLS loop of tensor_ops.irls_solve with exact inner solves: the first step reweights from f, every later one
    from the previous iterate.  Returns (iterates, energies): energies[0] is E(f), energies[k + 1] that of iterate k.
    perturb: None, or a relative residual -- every solve's result is then moved along a seeded random direction until
    |b - A u| = perturb * |b|, the error an inner solver that stops at that tolerance may leave."""
    f = _wide(f)
    H, W, C = f.shape
    rng = np.random.default_rng(seed)
    u, iterates = f, []
    energies = [energy(f, gx, gy, f, penalty, coupling, strength, eps, data_weight, per_channel)]
    for _ in range(outer):
        wx, wy = weights(u, gx, gy, penalty, coupling, strength, eps, per_channel=per_channel)
        new = np.empty_like(f)
        for c in range(C):
            wxc, wyc = (wx[:, :, c], wy[:, :, c]) if per_channel else (wx, wy)
            A, b = system(wxc, wyc, data_weight, None if gx is None else _wide(gx)[:, :, c], None if gy is None else _wide(gy)[:, :, c], f[:, :, c])
            x = np.linalg.solve(A, b)
            if perturb is not None:
                d = rng.standard_normal(x.size)
                x = x + d * (perturb * np.linalg.norm(b) / np.linalg.norm(A @ d))
            new[:, :, c] = x.reshape(H, W)
        u = new
        iterates.append(u)
        energies.append(energy(u, gx, gy, f, penalty, coupling, strength, eps, data_weight, per_channel))
    return iterates, energies


def step_image(W, H, C, seed, low=0.0, high=1.0, noise=0.05):
    """a two-level step image (the right part `high`, a lower-left block too) plus seeded Gaussian noise, H x W x C float64"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W, C), low)
    img[:, W // 2:] = high
    img[H // 2:, :W // 4] = high
    return img + noise * rng.standard_normal((H, W, C))
