"""Test-side expectations of CCP_MG_NULLSPACE_CONSTANT (include/ccp_gs.h), NOT product code.

A numpy model of the multigrid PCG of a weighted handle whose operator is floating (lambda = 0 everywhere, no fixed
pixel, every in-canvas edge weight > 0: singular, the constants its null space), on top of the V-cycles of
weighted_helpers (Galerkin), rescaled_helpers (rescaled), mixed_helpers (the fp32 V-cycle) and line_helpers (the line
smoother), which this file imports and does not change.  With n = W H and mean(v) = sum(v) / n:

    bm = mean(b);  m0 = mean(x);  r = (b - bm) - A x
    stop with 0 iterations if sqrt(r'r) < epsilon
    z = M r;  zm = mean(z);  rz = r'z - zm * sum(r);  p = z - zm
    loop: alpha = rz / p'Ap;  x += alpha p;  r += (-alpha) Ap;  stop if sqrt(r'r) < epsilon
          z = M r;  zm = mean(z);  rz' = r'z - zm * sum(r);  beta = rz' / rz;  p = (z - zm) + beta p
    end:  x += m0 - mean(x)

The device adds its sums up in another order (block partials), so the loop is compared to a tolerance and not bit for
bit; one V-cycle keeps the bits of the helper it comes from."""
import math

import numpy as np

import line_helpers as lh
import mixed_helpers as mh
import rescaled_helpers as rh
import weighted_helpers as wh

CS = {"galerkin": 2.0, "rescaled": 1.0}


def hierarchy(kind, W, H, wx=None, wy=None):
    """The levels of a floating operator (lambda = 0) of hierarchy kind `kind`."""
    return (rh if kind == "rescaled" else wh).hierarchy(W, H, wx, wy, None)


def preconditioner(levels, kind, nu=2, precision="f64", smoother="point"):
    """r -> M r: the V-cycle of the existing helper that models the mode (nu: the sweeps, as the device is given them)."""
    cs = CS[kind]
    if smoother == "line":
        return lambda r: lh.vcycle(levels, r, nu, cs)
    if precision == "f32":
        levels32 = mh.narrow(levels)
        return lambda r: mh.vcycle(levels32, r, nu, cs)
    if kind == "rescaled":
        return lambda r: rh.vcycle(levels, r, nu)
    return lambda r: wh.vcycle(levels, r, nu)


def line_levels(W, H):
    """The (W_k, H_k) of the levels the line smoother relaxes by lines: level 0 and every coarse level above the tail
    (line_helpers.tail_level: a side > 32)."""
    out = [(W, H)]
    while True:
        W, H = (W + 1) // 2, (H + 1) // 2
        if W <= lh.TAIL_SIDE and H <= lh.TAIL_SIDE:
            return out
        out.append((W, H))


def line_served(W, H):
    """Does CONSTANT mode serve the line smoother at W x H?  Not if a line-smoothed level has one row or one column: its
    one line along the canvas is the singular (floating) operator itself, and the exact line solve divides by zero."""
    return all(w > 1 and h > 1 for w, h in line_levels(W, H))


def mean(v):
    return float(np.sum(v)) / v.size


def projected_vcycle(M, b):
    """ccp_grid_mg_apply in CONSTANT mode: (z - mean(z), z, bm) with z = M (b - bm)."""
    bm = mean(b)
    z = M(b - bm)
    return z + (0.0 - mean(z)), z, bm


def pcg(A, M, b, epsilon, max_iteration, x0=None):
    """The loop above: (x, iterations, converged, last sqrt(r'r), bm).  A: a level 0 with `apply`; M: r -> z."""
    n = b.size
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    bm = mean(b)
    m0 = mean(x)

    def close(x):
        return x + (m0 - mean(x))

    r = (b - bm) - A.apply(x)
    norm = math.sqrt(float(np.sum(r * r)))
    if norm < epsilon:
        return close(x), 0, True, norm, bm

    def project(r):
        z = M(r)
        zm = float(np.sum(z)) / n
        return z, zm, float(np.sum(r * z)) - zm * float(np.sum(r))

    z, zm, rz = project(r)
    p = z - zm
    cnt = 0
    while cnt < max_iteration:
        ap = A.apply(p)
        alpha = rz / float(np.sum(p * ap))
        x = x + alpha * p
        r = r + (-alpha) * ap
        norm = math.sqrt(float(np.sum(r * r)))
        if norm < epsilon:
            return close(x), cnt, True, norm, bm
        z, zm, rz_new = project(r)
        beta = rz_new / rz
        rz = rz_new
        p = (z - zm) + beta * p
        cnt += 1
    return close(x), cnt, False, norm, bm


def plain_pcg(kind):
    """The existing loop of the same helpers (CCP_MG_NULLSPACE_NONE): pcg(levels, b, epsilon, max_iteration, nu, x0)."""
    return (rh if kind == "rescaled" else wh).pcg


# ---- dense and scipy forms (the checks of tests/test_neumann_helpers.py) ------------------------------------------------
def projector(n):
    """P = I - 1 1'/n: onto the mean-free vectors."""
    return np.eye(n) - np.full((n, n), 1.0 / n)


def projected_preconditioner_matrix(levels, kind, nu=2):
    """P M P as a dense matrix (M from the helper's preconditioner_matrix: one V-cycle per unit vector)."""
    M, live = (rh if kind == "rescaled" else wh).preconditioner_matrix(levels, nu)
    assert len(live) == levels[0].W * levels[0].H               # a floating operator has no dead pixel
    P = projector(len(live))
    return P @ M @ P


def reference_solve(level, b, x_mean):
    """The least-squares solution of the floating system A x = b with mean(x) = x_mean, by scipy's direct solve of the
    bordered system [[A, 1], [1', 0]] [x; mu] = [b; n x_mean]: mu takes mean(b), the part of b outside A's range."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    H, W = level.d.shape
    n = W * H
    one = sp.csr_matrix(np.ones((n, 1)))
    K = sp.bmat([[wh.matrix(level), one], [one.T, None]], format="csc")
    sol = sla.spsolve(K, np.concatenate([b.ravel(), [n * x_mean]]))
    return sol[:n].reshape(H, W), float(sol[n])


# ---- the systems of the tests -------------------------------------------------------------------------------------------
def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def weights(W, H, seed, lo=0.1, hi=10.0):
    """float32 edge weights uniform in [lo, hi)."""
    g = rng(seed)
    return g.uniform(lo, hi, (H, W)).astype(np.float32), g.uniform(lo, hi, (H, W)).astype(np.float32)


def guidance(W, H, seed, scale=1.0):
    """float32 gx, gy uniform in [-60 scale, 60 scale)."""
    g = rng(seed)
    return (g.uniform(-60.0 * scale, 60.0 * scale, (H, W)).astype(np.float32),
            g.uniform(-60.0 * scale, 60.0 * scale, (H, W)).astype(np.float32))


def system(kind, W, H, weighted, seed=1, scale=1.0):
    """(levels, b, wx, wy, gx, gy): the floating operator with unit (wx = wy = None) or random weights, and the consistent
    b = -div(w g) of random guidance."""
    wx, wy = weights(W, H, 100 + seed) if weighted else (None, None)
    levels = hierarchy(kind, W, H, wx, wy)
    gx, gy = guidance(W, H, seed, scale)
    return levels, wh.rhs(levels[0], gx, gy), wx, wy, gx, gy
