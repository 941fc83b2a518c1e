"""The numpy model of ccp_grid_reweight_robust_device (include/ccp_gs.h, "Robust data term"): lambda formed from |u - f| in
exactly the header's operation order, the edge weights with the one penalty that call adds ("quadratic": phi = 1.0), the
energy an IRLS loop on both minimises, a dense IRLS (np.linalg.solve) for tiny canvases and the outlier image the tests
denoise.  The edge weights of the other penalties come from reweight_helpers.weights, unchanged.

As there, every array operation is element-wise fp64, one correctly rounded operation per numpy call, and the channels are
accumulated by a python loop in channel order, so `data_weights` gives the bits the scalar loop `data_weights_scalar`
gives (tests/test_robust_helpers.py) and the bits the kernel must give (tests/test_gpu_robust.py)."""
import math

import numpy as np

import reweight_helpers as rh

PENALTIES = rh.PENALTIES + ("quadratic",)


def phi(q, penalty, eps):
    if penalty == "quadratic":
        return np.ones_like(np.asarray(q, dtype=np.float64))
    return rh.phi(q, penalty, eps)


def psi(rho, penalty, eps):
    """the penalty whose derivative is rho * phi(rho^2)"""
    if penalty == "quadratic":
        rho = np.asarray(rho, dtype=np.float64)
        return rho * rho / 2.0
    return rh.psi(rho, penalty, eps)


def data_residuals(u, f, per_channel):
    """dq: H x W x sets, the sum of (f - u)^2 over the channel set, in channel order from +0.0"""
    u = rh._wide(u)
    f = rh._wide(f, u.shape)
    H, W, C = u.shape
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    dq = np.zeros((H, W, len(sets)))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, chans in enumerate(sets):
            acc = np.zeros((H, W))
            for c in chans:
                r = f[:, :, c] - u[:, :, c]
                acc = acc + r * r
            dq[:, :, k] = acc
    return dq


def data_weights(u, f, penalty, scale, eps, base=None, per_channel=False):
    """lambda of the header's definition, float64: H x W for the shared operator, H x W x C for one per channel.  u, f:
    H x W x C of any dtype (widened exactly; f may be H x W: every channel's; f is not read for "quadratic"); base:
    H x W (x C) of float32 / float64, or None (lambda = t)."""
    u = rh._wide(u)
    H, W, C = u.shape
    sets = C if per_channel else 1
    scale = np.float64(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        if penalty == "quadratic":
            t = np.full((H, W, sets), scale * np.float64(1.0))
        else:
            t = scale * phi(data_residuals(u, f, per_channel), penalty, eps)
        lam = t if base is None else rh._wide(base, t.shape) * t
    lam = np.array(lam)
    return lam if per_channel else lam[:, :, 0]


def data_weights_scalar(u, f, penalty, scale, eps, base=None, per_channel=False):
    """`data_weights` as a scalar loop over y, x and the channels, one python float operation at a time: the header's
    text, line by line"""
    u = rh._wide(u)
    H, W, C = u.shape
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    lam = np.zeros((H, W, len(sets)))
    scale = float(scale)
    f = None if f is None else np.asarray(f)

    def phi1(q):
        if penalty == "charbonnier":
            return 1.0 / math.sqrt(q + float(eps) * float(eps))
        if penalty == "huber":
            return 1.0 / max(math.sqrt(q), float(eps))
        if penalty == "reciprocal":
            return 1.0 / (math.sqrt(q) + float(eps))
        return 1.0

    for k, chans in enumerate(sets):
        for y in range(H):
            for x in range(W):
                if penalty == "quadratic":
                    t = scale * 1.0
                else:
                    acc = 0.0
                    for c in chans:
                        fv = float(f[y, x]) if f.ndim == 2 else float(f[y, x, c])
                        r = fv - float(u[y, x, c])
                        acc += r * r
                    t = scale * phi1(acc)
                if base is None:
                    lam[y, x, k] = t
                else:
                    b = np.asarray(base)
                    lam[y, x, k] = (float(b[y, x]) if b.ndim == 2 else float(b[y, x, k])) * t
    return lam if per_channel else lam[:, :, 0]


def edge_weights(u, gx, gy, penalty, coupling, scale, eps, base_wx=None, base_wy=None, per_channel=False):
    """(wx, wy) as ccp_grid_reweight_robust_device forms them: reweight_helpers.weights, and for "quadratic" t = scale * 1.0,
    w = base * t or t on every edge that exists"""
    if penalty != "quadratic":
        return rh.weights(u, gx, gy, penalty, coupling, scale, eps, base_wx, base_wy, per_channel)
    if coupling not in rh.COUPLINGS:
        raise ValueError(coupling)
    H, W, C = np.asarray(u).shape
    shape = (H, W, C if per_channel else 1)
    t = np.full(shape, np.float64(scale) * np.float64(1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        wx = np.array(t if base_wx is None else rh._wide(base_wx, shape) * t)
        wy = np.array(t if base_wy is None else rh._wide(base_wy, shape) * t)
    wx[:, -1, :] = 0.0
    wy[-1, :, :] = 0.0
    return (wx, wy) if per_channel else (wx[:, :, 0], wy[:, :, 0])


def energy_robust(u, gx, gy, f, penalty, coupling, strength, eps, data_penalty, data_scale, data_eps, per_channel=False):
    """E(u) = sum 2 strength psi(rho) + sum 2 data_scale psi_d(delta) with unit base weights and base lambda 1: rho as
    reweight_helpers.energy's, delta^2 the sum of (u - f)^2 over the channel set ("quadratic": 2 psi_d = delta^2, the
    quadratic data term of reweight_helpers.energy)"""
    u, f = rh._wide(u), rh._wide(f)
    qx, qy = rh.residuals(u, gx, gy, per_channel)
    if coupling == "pixel":
        reg = psi(np.sqrt(qx + qy), penalty, eps).sum()
    else:
        reg = psi(np.sqrt(qx[:, :-1]), penalty, eps).sum() + psi(np.sqrt(qy[:-1]), penalty, eps).sum()
    data = psi(np.sqrt(data_residuals(u, f, per_channel)), data_penalty, data_eps).sum()
    return float(2.0 * strength * reg + 2.0 * data_scale * data)


def dense_irls_robust(f, gx, gy, penalty, coupling, strength, eps, data_penalty, data_scale, data_eps, outer, per_channel=False,
                      first_step="quadratic", perturb=None, seed=0):
    """reweight_helpers.dense_irls with lambda reweighted too, the loop of tensor_ops.irls_solve(data_penalty=...) with exact
    inner solves.  Step 0 reweights from u = f, where every data residual is 0: first_step "quadratic" gives it the
    quadratic data term (lambda = data_scale), "robust" the robust one (lambda = data_scale * phi_d(0)).  Returns
    (iterates, energies, lambdas): energies[0] is E(f), energies[k + 1] that of iterate k; lambdas[k] what step k solved
    with.  perturb, seed: as dense_irls's."""
    if first_step not in ("quadratic", "robust"):
        raise ValueError(first_step)
    f = rh._wide(f)
    H, W, C = f.shape
    rng = np.random.default_rng(seed)
    u, iterates, lambdas = f, [], []
    E = lambda v: energy_robust(v, gx, gy, f, penalty, coupling, strength, eps, data_penalty, data_scale, data_eps, per_channel)
    energies = [E(f)]
    for k in range(outer):
        wx, wy = edge_weights(u, gx, gy, penalty, coupling, strength, eps, per_channel=per_channel)
        dp = "quadratic" if k == 0 and first_step == "quadratic" else data_penalty
        lam = data_weights(u, f, dp, data_scale, data_eps, per_channel=per_channel)
        new = np.empty_like(f)
        for c in range(C):
            wxc, wyc, lc = (wx[:, :, c], wy[:, :, c], lam[:, :, c]) if per_channel else (wx, wy, lam)
            A, b = rh.system(wxc, wyc, lc, None if gx is None else rh._wide(gx)[:, :, c], None if gy is None else rh._wide(gy)[:, :, c], f[:, :, c])
            x = np.linalg.solve(A, b)
            if perturb is not None:
                d = rng.standard_normal(x.size)
                x = x + d * (perturb * np.linalg.norm(b) / np.linalg.norm(A @ d))
            new[:, :, c] = x.reshape(H, W)
        u = new
        iterates.append(u)
        lambdas.append(lam)
        energies.append(E(u))
    return iterates, energies, lambdas


# ---- the outlier image and the parameters of the denoising tests ------------------------------------------------------------
STRENGTH, EPS, DATA_SCALE, DATA_EPS, OUTER = 1.0, 1e-2, 1.0, 5e-2, 12
# (coupling, data penalty, one operator per channel): the two cases measured on the CPU
CASES = [("pixel", "charbonnier", False), ("edge", "huber", True)]


def outlier_image(W, H, C=2):
    """(clean, noisy): the step image of reweight_helpers.step_image (seed 1) without noise, and with noise 0.05 and 6 % of
    its samples replaced by -1 or 2 (the mask and the values from default_rng(5))"""
    clean = rh.step_image(W, H, C, seed=1, noise=0.0)
    noisy = rh.step_image(W, H, C, seed=1, noise=0.05)
    rng = np.random.default_rng(5)
    mask = rng.random((H, W, C)) < 0.06
    values = rng.integers(0, 2, size=(H, W, C)) * 3 - 1
    return clean, np.where(mask, values.astype(np.float64), noisy)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))
