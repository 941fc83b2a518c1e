"""Test-side expectations of the fp32 V-cycle (include/ccp_gs.h, CCP_MG_PRECISION_F32), NOT product code.

A float32 restatement of csrc/ccp_grid_mgs.hpp on top of mg_helpers / weighted_helpers / rescaled_helpers /
constrained_helpers, whose fp64 hierarchies it narrows:

* `narrow(levels)`: every level's d, we, ws (level 0 of a structured or mask handle: its diagonal) as float32, round to
  nearest; a pixel is live if its float32 d != 0.  The level classes' own sweep and residual then run on float32 arrays
  in the device's operation order -- every array they touch is float32, which `vcycle` checks at every step;
* `vcycle(levels32, b, nu, cs)`: b narrowed to float32 once, the V-cycle of mg_helpers (cs = 2.0) or of rescaled_helpers
  (cs = 1.0) with every value a float32, the result widened to float64;
* `pcg(levels, levels32, b, ...)`: the fp64 loop of mg_helpers.pcg (products with the fp64 level 0, numpy's dot
  products) preconditioned by that V-cycle.

`verdict(levels)` is the narrowing pass's check: False if a coefficient narrows to inf or a non-zero one to 0."""
import copy
import math

import numpy as np

import mg_helpers as mg

F32 = np.float32


def _f32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(F32)


def narrow(levels):
    out = []
    for lv in levels:
        n = copy.copy(lv)
        if isinstance(lv, mg.Level0):
            n.diag = _f32(lv.diag)                                  # small integers: exact
            n.live = n.diag != 0
        else:
            n.d, n.we, n.ws = _f32(lv.d), _f32(lv.we), _f32(lv.ws)
            n.live = n.d != 0
        out.append(n)
    return out


def verdict(levels):
    for lv in levels:
        for a in lv.coefficients():
            f = _f32(a)
            if not np.all(np.isfinite(f)) or np.any((np.asarray(a) != 0) & (f == 0)):
                return False
    return True


def _is32(*arrays):
    for a in arrays:
        assert a.dtype == F32, a.dtype


def _vcycle32(levels, b, nu, cs, k):
    lv = levels[k]
    _is32(b, *((lv.diag,) if isinstance(lv, mg.Level0) else lv.coefficients()))   # (a structured level 0 computes with diag alone)
    z = np.zeros_like(b)
    if k == len(levels) - 1:
        if k == 0:
            lv.sweep(z, b, mg.RED, first=True)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(lv.live, b / lv.d, F32(0.0))
        _is32(z)
        return z
    for s in range(nu):
        lv.sweep(z, b, mg.RED, first=(s == 0))
        lv.sweep(z, b, mg.BLACK)
    _is32(z)
    r = lv.residual(z, b)
    rc = mg.restrict(r)
    _is32(r, rc)
    e = _vcycle32(levels, rc, nu, cs, k + 1)
    up = np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)[:lv.H, :lv.W]
    z = np.where(lv.live, z + F32(cs) * up, z)
    _is32(z)
    for _ in range(nu):
        lv.sweep(z, b, mg.BLACK)
        lv.sweep(z, b, mg.RED)
    _is32(z)
    return z


def vcycle(levels32, b, nu=2, cs=2.0):
    """z = M32^-1 b: float64 in, float64 out, float32 in between."""
    with np.errstate(over="ignore"):
        b32 = np.asarray(b, dtype=np.float64).astype(F32)
    return _vcycle32(levels32, b32, nu, cs, 0).astype(np.float64)


def pcg(levels, levels32, b, epsilon, max_iteration, nu=2, cs=2.0, x0=None):
    """(x, iterations, converged, last sqrt(r'r)): mg_helpers.pcg in fp64 with the float32 V-cycle as M^-1."""
    A = levels[0]
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A.apply(x)
    rr = float(np.sum(r * r))
    if math.sqrt(rr) < epsilon:
        return x, 0, True, math.sqrt(rr)
    z = vcycle(levels32, r, nu, cs)
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
        z = vcycle(levels32, r, nu, cs)
        rz_new = float(np.sum(r * z))
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        cnt += 1
    return x, cnt, False, norm


def preconditioner_matrix(levels32, nu=2, cs=2.0):
    """weighted_helpers.preconditioner_matrix's method on this file's V-cycle."""
    lv = levels32[0]
    live = np.flatnonzero(lv.live.ravel())
    M = np.zeros((len(live), len(live)))
    for j, i in enumerate(live):
        e = np.zeros(lv.W * lv.H)
        e[i] = 1.0
        M[:, j] = vcycle(levels32, e.reshape(lv.H, lv.W), nu, cs).ravel()[live]
    return M, live


# ---- the systems of tests/test_mixed_helpers.py and tests/test_gpu_mixed.py ----------------------------------------------
def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def field(W, H, seed, lo=-60.0, hi=60.0):
    return rng(seed).uniform(lo, hi, (H, W)).astype(np.float32)


def ellipse_fixed(W, H):
    """Fixed = everything outside an ellipse that reaches the left and right canvas borders."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx - (W - 1) / 2) / (0.55 * W)) ** 2 + ((yy - (H - 1) / 2) / (0.35 * H)) ** 2 >= 1.0).astype(np.uint8)


def disc_and_blob(W, H):
    """A disc around the centre plus a detached blob near the top left corner (u8; a 1-pixel image is all region)."""
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.33 * min(W, H)
    m = (xx - W / 2.0) ** 2 + (yy - H / 2.0) ** 2 <= max(r * r, 1.0)
    if min(W, H) >= 30:
        m[2:2 + H // 10, 3:3 + W // 10] = True
    if W * H == 1:
        m[:] = True
    return m.astype(np.uint8)


def patch_image(W, H, seed=7):
    """Flat 16-px patches with hard edges plus a little noise, three channels, as float64 whole numbers in [0, 255]
    (tools/weighted_bench.py's image, from numpy's generator).  A deliberate deviation: tests/test_gpu_rescaled.py's WLS
    test draws that image from a torch generator on the device, which a CPU test cannot do, so this is the same
    construction (patch size, amplitudes, seed) with numpy's generator -- other random numbers, not the same pixels, and
    not one of synth.py's images either.  The
    cap the test holds it to is unchanged (1.1 x the fp64 count + 1); NOTES R16.1 has the counts of a harsher image too."""
    g = rng(seed)
    patches = g.uniform(size=(H // 16 + 1, W // 16 + 1, 3))
    img = patches.repeat(16, 0).repeat(16, 1)[:H, :W] * 230.0 + 25.0 * g.uniform(size=(H, W, 3))
    return np.floor(np.clip(img, 0, 255))


def wls_weights(img, lam=1.0, alpha=1.2, eps=1e-4):
    """tensor_ops.wls_weights in numpy for an H x W x C image in [0, 255] (the luminance is the channel mean): float64
    H x W."""
    ell = np.log(img.mean(axis=-1) / 255.0 + eps)
    wx, wy = np.zeros_like(ell), np.zeros_like(ell)
    wx[:, :-1] = lam / (np.abs(ell[:, 1:] - ell[:, :-1]) ** alpha + eps)
    wy[:-1, :] = lam / (np.abs(ell[1:, :] - ell[:-1, :]) ** alpha + eps)
    return wx, wy


def pcg_system(name, W, H):
    """(levels, b, x0, cs, what the handle needs) of a named MG-PCG case: "screened" (lambda 1e-2, rescaled),
    "constrained" (the ellipse free, the rest fixed, lambda 1e-2, rescaled), "solve_channel" (the structured handle's
    matrix), "mask" (the Dirichlet Laplacian on disc_and_blob), "wls" (lambda 1, alpha 1.2 on patch_image, rescaled)."""
    import constrained_helpers as ch
    import rescaled_helpers as rh
    import weighted_helpers as wh
    gx, gy, f = field(W, H, 1), field(W, H, 2), field(W, H, 3, 0.0, 255.0)
    if name == "screened":
        lam = np.full((H, W), 1e-2, np.float32)
        levels = rh.hierarchy(W, H, None, None, lam)
        return levels, wh.rhs(levels[0], gx, gy, f), f.astype(np.float64), 1.0, dict(lam=lam, gx=gx, gy=gy, f=f)
    if name == "constrained":
        lam = np.full((H, W), 1e-2, np.float32)
        fixed, v = ellipse_fixed(W, H), field(W, H, 4, -30.0, 290.0)
        levels = ch.hierarchy(W, H, None, None, lam, fixed, "rescaled")
        x0 = ch.x_after(levels[0], np.zeros((H, W)), f, v, init=True)
        return levels, ch.rhs(levels[0], gx, gy, f, v), x0, 1.0, dict(lam=lam, fixed=fixed, gx=gx, gy=gy, f=f, v=v)
    if name == "solve_channel":
        levels = mg.hierarchy(W, H)
        return levels, levels[0].apply(rng(11).uniform(0.0, 255.0, (H, W))), np.zeros((H, W)), 2.0, {}
    if name == "mask":
        m = disc_and_blob(W, H)
        levels = mg.hierarchy(W, H, m)
        return levels, levels[0].apply(np.where(m != 0, rng(12).uniform(0.0, 255.0, (H, W)), 0.0)), np.zeros((H, W)), 2.0, dict(mask=m)
    if name == "wls":
        img = patch_image(W, H)
        wx, wy = wls_weights(img)
        lam, f = np.ones((H, W)), img[..., 0].copy()                # channel 0 of the smoothing
        levels = rh.hierarchy(W, H, wx, wy, lam)
        return levels, wh.rhs(levels[0], None, None, f), f.copy(), 1.0, dict(wx=wx, wy=wy, lam=lam, f=f)
    raise KeyError(name)
