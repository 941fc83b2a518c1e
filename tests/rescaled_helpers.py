"""Test-side expectations of the rescaled hierarchy of weighted grid handles (include/ccp_gs.h,
CCP_MG_HIERARCHY_RESCALED), NOT product code.

A numpy restatement of k_weighted_coarsen with the edge factor 0.5 and of the V-cycle with the unscaled coarse
correction, in the device's operation order (as weighted_helpers.py and mg_helpers.py, which this file imports):

* level 0 is weighted_helpers' level 0 (d, we, ws, lam), unchanged;
* coarsening: lam_c = (l00 + l10) + (l01 + l11); each side = 0.5 * (sum of the two fine edge weights that leave the
  aggregate there); d_c = lam_c; += north; += west; += east; += south; we_c = east; ws_c = south;
* the V-cycle is mg_helpers.vcycle's with z += e_c (no factor) on live pixels.
"""
import math

import numpy as np

import mg_helpers as mg
import weighted_helpers as wh


def coarsen(level):
    """k_weighted_coarsen with edge = 0.5: the edge weights halved, lam summed."""
    lam, we, ws = (mg._pad_even(a) for a in (level.lam, level.we, level.ws))
    wsp = np.zeros((lam.shape[0] + 1, lam.shape[1]))
    wsp[1:, :] = ws
    wep = np.zeros((lam.shape[0], lam.shape[1] + 1))
    wep[:, 1:] = we
    lc = (lam[0::2, 0::2] + lam[0::2, 1::2]) + (lam[1::2, 0::2] + lam[1::2, 1::2])
    north = 0.5 * (wsp[0:-1:2, 0::2] + wsp[0:-1:2, 1::2])
    west = 0.5 * (wep[0::2, 0:-1:2] + wep[1::2, 0:-1:2])
    east = 0.5 * (we[0::2, 1::2] + we[1::2, 1::2])
    south = 0.5 * (ws[1::2, 0::2] + ws[1::2, 1::2])
    d = lc.copy()
    d = d + north
    d = d + west
    d = d + east
    d = d + south
    return wh.Coarse(d, east, south, lc)


def hierarchy(W, H, wx=None, wy=None, lam=None):
    levels = [wh.Level0(*wh.coefficients(W, H, wx, wy, lam))]
    while levels[-1].W > 1 or levels[-1].H > 1:
        levels.append(coarsen(levels[-1]))
    return levels


def vcycle(levels, b, nu=2, k=0):
    """z = M^-1 b on level k: mg_helpers.vcycle with the coarse correction added unscaled."""
    lv = levels[k]
    z = np.zeros_like(b)
    if k == len(levels) - 1:
        if k == 0:
            lv.sweep(z, b, mg.RED, first=True)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(lv.live, b / lv.d, 0.0)
        return z
    for s in range(nu):
        lv.sweep(z, b, mg.RED, first=(s == 0))
        lv.sweep(z, b, mg.BLACK)
    e = vcycle(levels, mg.restrict(lv.residual(z, b)), nu, k + 1)
    up = np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)[:lv.H, :lv.W]
    z = np.where(lv.live, z + up, z)
    for _ in range(nu):
        lv.sweep(z, b, mg.BLACK)
        lv.sweep(z, b, mg.RED)
    return z


def pcg(levels, b, epsilon, max_iteration, nu=2, x0=None):
    """mg_helpers.pcg with this file's V-cycle: (x, iterations, converged, last sqrt(r'r))."""
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


def preconditioner_matrix(levels, nu=2):
    """weighted_helpers.preconditioner_matrix's method on this file's V-cycle."""
    lv = levels[0]
    live = np.flatnonzero(lv.live.ravel())
    M = np.zeros((len(live), len(live)))
    for j, i in enumerate(live):
        e = np.zeros(lv.W * lv.H)
        e[i] = 1.0
        M[:, j] = vcycle(levels, e.reshape(lv.H, lv.W), nu).ravel()[live]
    return M, live
