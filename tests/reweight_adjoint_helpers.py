"""The numpy model of ccp_grid_reweight_adjoint_device (include/ccp_gs.h, "Backpropagating through a reweight"): the
vector-Jacobian product of reweight_helpers.weights and robust_helpers.data_weights in exactly the header's operation
order, its scalar-loop twin, and the gradient of a dense unrolled IRLS loop obtained by chaining it with
adjoint_helpers.dense_reference.

As in reweight_helpers, every array operation is element-wise fp64, one correctly rounded operation per numpy call, and
the channels run in a python loop in channel order, so `vjp` gives the bits `vjp_scalar` gives
(tests/test_reweight_adjoint_helpers.py) and the bits the kernel must give (tests/test_gpu_reweight_adjoint.py)."""
import math

import numpy as np

import adjoint_helpers as ah
import reweight_helpers as rh
import robust_helpers as bh

OUTPUTS = ("g_u", "g_gx", "g_gy", "g_f", "g_base_wx", "g_base_wy", "g_lambda")


def psi(q, phi, penalty, eps):
    """psi with d phi / d r_c = psi * r_c, from q and the phi the forward formed of it"""
    eps = np.float64(eps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if penalty == "charbonnier":
            p = phi * phi
            return -(p * phi)
        if penalty == "huber":
            return np.where(np.sqrt(q) > eps, -((phi * phi) * phi), 0.0)
        if penalty == "reciprocal":
            return np.where(q > 0.0, -((phi * phi) / np.sqrt(q)), 0.0)
        if penalty == "quadratic":
            return np.zeros_like(np.asarray(q, dtype=np.float64))
    raise ValueError(penalty)


def _plane(a, H, W, k):
    """set k's H x W plane of an optional H x W (x sets) array, widened exactly (None stays None)"""
    if a is None:
        return None
    a = np.asarray(a).astype(np.float64)
    return np.broadcast_to(a if a.ndim == 2 else a[:, :, k], (H, W))


def vjp(u, gx, gy, penalty, coupling, scale, eps, base_wx=None, base_wy=None, per_channel=False, grad_wx=None, grad_wy=None,
        data=None, grad_lambda=None):
    """Every output of the adjoint pass as float64 arrays: g_u, g_gx, g_gy, g_f H x W x C; g_base_wx, g_base_wy, g_lambda
    H x W for the shared operator and H x W x C for one per channel.  The forward's arguments as reweight_helpers.weights
    takes them (penalty may be "quadratic" with `data`); grad_wx, grad_wy, grad_lambda: the upstream gradients, shaped as
    the weights, None: +0.0.  data: None (the plain reweight: g_f and g_lambda are None) or a dict with f, penalty, scale,
    eps and base (the base lambda, None: 1)."""
    if coupling not in rh.COUPLINGS:
        raise ValueError(coupling)
    u = rh._wide(u)
    H, W, C = u.shape
    gxw, gyw = rh._wide(gx, u.shape), rh._wide(gy, u.shape)
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    S = len(sets)
    scale = np.float64(scale)
    out = {n: np.zeros((H, W, C)) for n in ("g_u", "g_gx", "g_gy")}
    out.update({n: np.zeros((H, W, S)) for n in ("g_base_wx", "g_base_wy")})
    out["g_f"] = out["g_lambda"] = None
    if data is not None:
        f = rh._wide(data.get("f"), u.shape)
        if f is None:
            f = np.zeros(u.shape)
        dscale = np.float64(data["scale"])
        out["g_f"], out["g_lambda"] = np.zeros((H, W, C)), np.zeros((H, W, S))
    if penalty == "quadratic":
        qx_all = qy_all = np.zeros((H, W, S))
    else:
        qx_all, qy_all = rh.residuals(u, gx, gy, per_channel)
    zero = np.zeros((H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, chans in enumerate(sets):
            qx, qy = qx_all[:, :, k], qy_all[:, :, k]
            Gx, Gy = _plane(grad_wx, H, W, k), _plane(grad_wy, H, W, k)
            Gx, Gy = zero if Gx is None else Gx, zero if Gy is None else Gy
            bx, by = _plane(base_wx, H, W, k), _plane(base_wy, H, W, k)
            ax = Gx if bx is None else Gx * bx
            ay = Gy if by is None else Gy * by
            if coupling == "pixel":
                q = qx + qy
                phix = phiy = bh.phi(q, penalty, eps)
                a = np.zeros((H, W))
                a[:, :-1] = a[:, :-1] + ax[:, :-1]
                a[:-1] = a[:-1] + ay[:-1]
                kx = ky = (a * scale) * psi(q, phix, penalty, eps)
            else:
                phix, phiy = bh.phi(qx, penalty, eps), bh.phi(qy, penalty, eps)
                kx = (ax * scale) * psi(qx, phix, penalty, eps)
                ky = (ay * scale) * psi(qy, phiy, penalty, eps)
            out["g_base_wx"][:, :-1, k] = (Gx * (scale * phix))[:, :-1]
            out["g_base_wy"][:-1, :, k] = (Gy * (scale * phiy))[:-1]
            if data is not None:
                Gl = _plane(grad_lambda, H, W, k)
                Gl = zero if Gl is None else Gl
                bl = _plane(data.get("base"), H, W, k)
                if data["penalty"] == "quadratic":
                    dq = np.zeros((H, W))
                else:
                    dq = bh.data_residuals(u[:, :, chans], f[:, :, chans], False)[:, :, 0]
                phid = bh.phi(dq, data["penalty"], data["eps"])
                kd = ((Gl if bl is None else Gl * bl) * dscale) * psi(dq, phid, data["penalty"], data["eps"])
                out["g_lambda"][:, :, k] = Gl * (dscale * phid)
            for c in chans:
                uc = u[:, :, c]
                rx = (gxw[:, :-1, c] if gxw is not None else np.zeros((H, W - 1))) - (uc[:, 1:] - uc[:, :-1])
                ry = (gyw[:-1, :, c] if gyw is not None else np.zeros((H - 1, W))) - (uc[1:] - uc[:-1])
                e, s = kx[:, :-1] * rx, ky[:-1] * ry
                out["g_gx"][:, :-1, c] = e
                out["g_gy"][:-1, :, c] = s
                t = np.zeros((H, W))
                t[:, :-1] = t[:, :-1] + e
                t[:-1] = t[:-1] + s
                t[:, 1:] = t[:, 1:] - e
                t[1:] = t[1:] - s
                if data is not None:
                    gf = kd * (f[:, :, c] - uc)
                    out["g_f"][:, :, c] = gf
                    t = t - gf
                out["g_u"][:, :, c] = t
    if not per_channel:
        for n in ("g_base_wx", "g_base_wy", "g_lambda"):
            out[n] = None if out[n] is None else out[n][:, :, 0]
    return out


def _psi1(q, phi, penalty, eps):
    if penalty == "charbonnier":
        p = phi * phi
        return -(p * phi)
    if penalty == "huber":
        return -((phi * phi) * phi) if math.sqrt(q) > eps else 0.0
    if penalty == "reciprocal":
        return -((phi * phi) / math.sqrt(q)) if q > 0.0 else 0.0
    return 0.0


def _phi1(q, penalty, eps):
    if penalty == "charbonnier":
        return 1.0 / math.sqrt(q + eps * eps)
    if penalty == "huber":
        return 1.0 / max(math.sqrt(q), eps)
    if penalty == "reciprocal":
        return 1.0 / (math.sqrt(q) + eps)
    return 1.0


def vjp_scalar(u, gx, gy, penalty, coupling, scale, eps, base_wx=None, base_wy=None, per_channel=False, grad_wx=None, grad_wy=None,
               data=None, grad_lambda=None):
    """`vjp` as a scalar loop over y, x and the channels, one python float operation at a time: the header's text, line
    by line (finite inputs only: python raises where numpy would give inf)"""
    u = rh._wide(u)
    H, W, C = u.shape
    sets = [[c] for c in range(C)] if per_channel else [list(range(C))]
    S = len(sets)
    scale, eps = float(scale), float(eps)
    out = {n: np.zeros((H, W, C)) for n in ("g_u", "g_gx", "g_gy")}
    out.update({n: np.zeros((H, W, S)) for n in ("g_base_wx", "g_base_wy")})
    out["g_f"] = out["g_lambda"] = None
    if data is not None:
        out["g_f"], out["g_lambda"] = np.zeros((H, W, C)), np.zeros((H, W, S))
        f = None if data.get("f") is None else np.asarray(data["f"])
        dpen, dscale, deps = data["penalty"], float(data["scale"]), float(data["eps"]) if data.get("eps") is not None else 1.0

    def at(a, y, x, k, absent):
        if a is None:
            return absent
        a = np.asarray(a)
        return float(a[y, x]) if a.ndim == 2 else float(a[y, x, k])

    def rx(y, x, c):
        return at(gx, y, x, c, 0.0) - (float(u[y, x + 1, c]) - float(u[y, x, c]))

    def ry(y, x, c):
        return at(gy, y, x, c, 0.0) - (float(u[y + 1, x, c]) - float(u[y, x, c]))

    def edge_k(y, x, k, chans):
        """(k_x, k_y, phi_x, phi_y) of pixel (x, y) of set k"""
        he, hs = x + 1 < W, y + 1 < H
        qx = qy = 0.0
        if penalty != "quadratic":
            if he:
                for c in chans:
                    r = rx(y, x, c)
                    qx += r * r
            if hs:
                for c in chans:
                    r = ry(y, x, c)
                    qy += r * r
        Gx, Gy = at(grad_wx, y, x, k, 0.0), at(grad_wy, y, x, k, 0.0)
        bx, by = at(base_wx, y, x, k, None), at(base_wy, y, x, k, None)
        ax = Gx if bx is None else Gx * bx
        ay = Gy if by is None else Gy * by
        if coupling == "pixel":
            q = qx + qy
            phix = phiy = _phi1(q, penalty, eps)
            a = 0.0
            if he:
                a += ax
            if hs:
                a += ay
            kx = ky = (a * scale) * _psi1(q, phix, penalty, eps)
        else:
            phix, phiy = _phi1(qx, penalty, eps), _phi1(qy, penalty, eps)
            kx = (ax * scale) * _psi1(qx, phix, penalty, eps)
            ky = (ay * scale) * _psi1(qy, phiy, penalty, eps)
        return kx, ky, phix, phiy, Gx, Gy

    for k, chans in enumerate(sets):
        for y in range(H):
            for x in range(W):
                he, hs = x + 1 < W, y + 1 < H
                kx, ky, phix, phiy, Gx, Gy = edge_k(y, x, k, chans)
                if he:
                    out["g_base_wx"][y, x, k] = Gx * (scale * phix)
                if hs:
                    out["g_base_wy"][y, x, k] = Gy * (scale * phiy)
                kW = edge_k(y, x - 1, k, chans)[0] if x >= 1 else 0.0
                kN = edge_k(y - 1, x, k, chans)[1] if y >= 1 else 0.0
                if data is not None:
                    fv = lambda c: 0.0 if f is None else (float(f[y, x]) if f.ndim == 2 else float(f[y, x, c]))
                    dq = 0.0
                    if dpen != "quadratic":
                        for c in chans:
                            d = fv(c) - float(u[y, x, c])
                            dq += d * d
                    phid = _phi1(dq, dpen, deps)
                    Gl = at(grad_lambda, y, x, k, 0.0)
                    bl = at(data.get("base"), y, x, k, None)
                    kd = ((Gl if bl is None else Gl * bl) * dscale) * _psi1(dq, phid, dpen, deps)
                    out["g_lambda"][y, x, k] = Gl * (dscale * phid)
                for c in chans:
                    t = 0.0
                    if he:
                        e = kx * rx(y, x, c)
                        out["g_gx"][y, x, c] = e
                        t += e
                    if hs:
                        s = ky * ry(y, x, c)
                        out["g_gy"][y, x, c] = s
                        t += s
                    if x >= 1:
                        t -= kW * rx(y, x - 1, c)
                    if y >= 1:
                        t -= kN * ry(y - 1, x, c)
                    if data is not None:
                        gf = kd * (fv(c) - float(u[y, x, c]))
                        out["g_f"][y, x, c] = gf
                        t -= gf
                    out["g_u"][y, x, c] = t
    if not per_channel:
        for n in ("g_base_wx", "g_base_wy", "g_lambda"):
            out[n] = None if out[n] is None else out[n][:, :, 0]
    return out


def margins(u, gx, gy, eps, data=None, per_channel=False):
    """The input condition of the difference tests, asked of the reference alone: (the smallest |sqrt(q) - eps| and the
    smallest q) over every edge and pixel argument of phi, both couplings, the data residual included"""
    qx, qy = rh.residuals(u, gx, gy, per_channel)
    owner = np.ones(qx.shape, bool)
    owner[-1, -1] = False                                    # the last pixel owns no edge: its q is not an argument of phi
    qs = [qx[:, :-1].ravel(), qy[:-1].ravel(), (qx + qy)[owner]]
    gaps = [np.abs(np.sqrt(q) - eps) for q in qs]
    if data is not None and data["penalty"] != "quadratic":
        dq = bh.data_residuals(u, rh._wide(data["f"], rh._wide(u).shape), per_channel).ravel()
        qs.append(dq)
        gaps.append(np.abs(np.sqrt(dq) - data["eps"]))
    return float(min(g.min() for g in gaps if g.size)), float(min(q.min() for q in qs if q.size))


# ---- the gradient of an unrolled dense IRLS loop ---------------------------------------------------------------------------
def dense_unrolled(f, gx, gy, penalty, coupling, strength, eps, outer, data_weight=1.0, base_wx=None, base_wy=None, values=None, fixed=None,
                   data_penalty=None, data_eps=None, first_step="quadratic", solve=None):
    """The loop of tensor_ops.irls_solve_grad on a shared operator with exact inner solves.  Returns (iterates, steps):
    steps[k] = (u_in, wx, wy, lam, data) of step k -- the image it reweighted from, what it solved with and the `data`
    dict its reweight took (None: lambda passed through).  data_weight: a number or an H x W array, the quadratic lambda
    (data_penalty None) or the base lambda of the robust one.  solve: dense_solve's replacement (same arguments)."""
    f = rh._wide(f)
    H, W, C = f.shape
    solve = solve or ah.dense_solve
    lam0 = np.broadcast_to(np.asarray(data_weight, dtype=np.float64), (H, W))
    u, iterates, steps = f, [], []
    for k in range(outer):
        data = None
        if data_penalty is not None:
            dp = "quadratic" if k == 0 and first_step == "quadratic" else data_penalty
            data = dict(f=f, penalty=dp, scale=1.0, eps=data_eps, base=lam0)
        wx, wy = bh.edge_weights(u, gx, gy, penalty, coupling, strength, eps, base_wx, base_wy)
        lam = lam0 if data is None else bh.data_weights(u, f, data["penalty"], 1.0, data_eps, base=lam0)
        steps.append((u, wx, wy, lam, data))
        u = solve(gx, gy, f, wx, wy, lam, values, fixed, shape=(H, W, C))
        iterates.append(u)
    return iterates, steps


def dense_unrolled_gradients(grad, f, gx, gy, penalty, coupling, strength, eps, outer, reference=None, **kw):
    """The gradients of L = sum grad * u_K of dense_unrolled's last iterate with respect to f, gx, gy, values, the base
    weights and data_weight (as an H x W plane), by chaining adjoint_helpers.dense_reference with `vjp` backwards through
    the steps.  reference: dense_reference's replacement (same arguments; the PCG model of the tolerance measurement).
    Returns (u_K, {"f", "gx", "gy", "values", "base_wx", "base_wy", "data_weight"})."""
    reference = reference or ah.dense_reference
    values, fixed = kw.get("values"), kw.get("fixed")
    base_wx, base_wy = kw.get("base_wx"), kw.get("base_wy")
    iterates, steps = dense_unrolled(f, gx, gy, penalty, coupling, strength, eps, outer, **kw)
    H, W, C = iterates[-1].shape
    total = {n: np.zeros((H, W, C)) for n in ("f", "gx", "gy", "values")}
    total.update({n: np.zeros((H, W)) for n in ("base_wx", "base_wy", "data_weight")})
    G = np.asarray(grad, dtype=np.float64)
    for k in range(outer - 1, -1, -1):
        u_in, wx, wy, lam, data = steps[k]
        got = reference(G, gx, gy, f, wx, wy, lam, values, fixed)[2]
        for n in ("f", "gx", "gy", "values"):
            total[n] += got[n]
        back = vjp(u_in, gx, gy, penalty, coupling, strength, eps, base_wx, base_wy, False, got["wx"], got["wy"], data,
                   got["lam"] if data is not None else None)
        total["gx"] += back["g_gx"]
        total["gy"] += back["g_gy"]
        total["base_wx"] += back["g_base_wx"]
        total["base_wy"] += back["g_base_wy"]
        if data is None:
            total["data_weight"] += got["lam"]
        else:
            total["f"] += back["g_f"]
            total["data_weight"] += back["g_lambda"]
        if k == 0:
            total["f"] += back["g_u"]                        # step 0 reweights from f
        G = back["g_u"]
    return iterates[-1], total
