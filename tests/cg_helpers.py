"""Test-side expectations of conjugate gradient (ccp_*_conjugate_gradient, ccp_csr_conjugate_gradient_jacobi), NOT product code.

`conjugate_gradient` and `conjugate_gradient_jacobi` restate SparseMatrix::conjugateGradient (sparse-matrix.h:396-434) and
::conjugateGradientEigen (:494-535) the way orc_conjugate_gradient / orc_conjugate_gradient_jacobi in oracle/ccp_oracle.c
do, in numpy, and also return the history of sqrt(r1len) — what a report's last_l1_step holds after the last update.  The
products A v are the oracle's own (applyToVector's order); the dot products are numpy's, so x agrees with the oracle to
rounding, not bit for bit.

Stops are placed as in stop_rule_helpers.py: from x0 = 0 (or x0 scaled with b) the residuals of s b are s times those of
b, so a per-channel scale s moves a channel's norm sequence past one shared epsilon.  CG norms are not monotone: a stop can
only be placed at an update whose norm is a new running minimum (`eligible`).  The placement is only a guess; tests read
the expected stop off the oracle's own run of the scaled system.

`first_iteration_ld` evaluates the first update in np.longdouble: a reference with no summation-order question."""
import math

import numpy as np

MARGIN = 1e-6        # every checked norm at least this far (relative) from epsilon: the device's sums are tree-ordered


def conjugate_gradient(apply, b, epsilon, max_iteration, init=None):
    """(x, iterations, converged, norms): the loop of sparse-matrix.h:396-434; iterations is the reference's `cnt`,
    norms[k-1] = sqrt(r1len) after update k (one per update run, the stopping one included)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if init is None else np.array(init, dtype=np.float64)   # :397,401-403
    r = b - apply(x)                                                             # :406-407
    p = r.copy()                                                                 # :410
    cnt, norms = 0, []
    while cnt < max_iteration:
        rlen = float(r @ r)                                                      # :418
        ap = apply(p)                                                            # :419
        alpha = rlen / float(p @ ap)                                             # :420
        x = x + alpha * p                                                        # :421
        r1 = r + (-alpha) * ap                                                   # :422
        r1len = float(r1 @ r1)                                                   # :423
        norms.append(math.sqrt(r1len))
        if math.sqrt(r1len) < epsilon:                                           # :425
            return x, cnt, True, np.array(norms)
        beta = r1len / rlen                                                      # :426
        p = r1 + beta * p                                                        # :427
        r = r1                                                                   # :429
        cnt += 1
    return x, cnt, False, np.array(norms)


def jacobi_inverse(values, col, rowp):
    """extractDiagnolColInv (sparse-matrix.h:472-491): 1/a_ii of the first stored diagonal entry, 1 if absent or 0."""
    n = len(rowp) - 1
    rows = np.repeat(np.arange(n), np.diff(rowp))
    inv = np.ones(n)
    on = np.flatnonzero(col == rows)
    first = on[np.unique(rows[on], return_index=True)[1]]
    v = values[first]
    nz = v != 0.0
    inv[rows[first][nz]] = 1.0 / v[nz]
    return inv


def conjugate_gradient_jacobi(apply, inv, b, epsilon, max_iteration):
    """(x, iterations, converged, norms) of sparse-matrix.h:494-535 (x0 = 0); norms[k-1] = sqrt(error) after update k."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)                                                         # :495
    r = b - apply(x)                                                             # :500-501
    p = r * inv                                                                  # :503
    olddist = float(p @ r)                                                       # :508
    cnt, norms = 0, []
    while cnt < max_iteration:
        ap = apply(p)                                                            # :516
        alpha = olddist / float(p @ ap)                                          # :517
        x = x + alpha * p                                                        # :518
        r = r + (-alpha) * ap                                                    # :519
        error = float(r @ r)                                                     # :520
        norms.append(math.sqrt(error))
        if math.sqrt(error) < epsilon:                                           # :521
            return x, cnt, True, np.array(norms)
        z = r * inv                                                              # :522
        newdist = float(z @ r)                                                   # :523
        beta = newdist / olddist                                                 # :524
        olddist = newdist                                                        # :525
        p = z + beta * p                                                         # :526
        cnt += 1                                                                 # :528
    return x, cnt, False, np.array(norms)


# ---- stop placement -------------------------------------------------------------------------------------------------
def expected_stop(norms, epsilon, max_iteration):
    """(iterations, converged, last norm) of the loop on this norm sequence: the first update k whose norm is below
    epsilon stops it with cnt = k - 1; otherwise max_iteration updates run."""
    for k in range(1, max_iteration + 1):
        if norms[k - 1] < epsilon:
            return k - 1, 1, float(norms[k - 1])
    return max_iteration, 0, float(norms[max_iteration - 1]) if max_iteration else 0.0


def eligible(norms):
    """The updates k (1-based) a stop can be placed at: norm k lies below every earlier norm by a factor that leaves
    MARGIN on both sides of epsilon when s * epsilon sits at their geometric mean."""
    out, low = [], math.inf
    for k, v in enumerate(norms, start=1):
        if v * (1 + MARGIN) ** 2 < low:
            out.append(k)
        low = min(low, v)
    return out


def nearest_eligible(norms, want, taken=()):
    ks = [k for k in eligible(norms) if k not in taken]
    return min(ks, key=lambda k: (abs(k - want), k))


def scale_for(norms, target, epsilon):
    """s such that s * norms first falls below epsilon at update `target` (None: never within len(norms)), with
    epsilon at the geometric mean of the two norms that decide it."""
    if target is None:
        return 4.0 * epsilon / float(np.min(norms))
    assert target in eligible(norms), (target, "not an eligible stop")
    lo = float(norms[target - 1])
    before = norms[:target - 1]
    if len(before) == 0:
        return epsilon / (4.0 * lo)
    return epsilon / math.sqrt(lo * float(np.min(before)))


def clear_of(norms, epsilon, upto):
    """Every norm up to update `upto` lies at least MARGIN (relative) away from epsilon."""
    return all(abs(v - epsilon) >= MARGIN * epsilon for v in norms[:upto])


# ---- long-double first update ---------------------------------------------------------------------------------------
def csr_apply_ld(values, col, rowp, v):
    """A v of a compressed CSR matrix, products and sums in np.longdouble."""
    n = len(rowp) - 1
    v = np.asarray(v, dtype=np.longdouble)
    prod = np.asarray(values, dtype=np.longdouble) * v[col]
    out = np.zeros(n, dtype=np.longdouble)
    ne = np.flatnonzero(np.diff(rowp) > 0)            # (reduceat needs non-empty segments)
    if len(ne):
        out[ne] = np.add.reduceat(prod, np.asarray(rowp)[ne])
    return out


def first_iteration_ld(values, col, rowp, b, x0=None):
    """(x_1, ||r_1||) of the first update from x0 (0 when None) in np.longdouble: r_0 = b - A x0, p_0 = r_0,
    alpha_1 = r_0'r_0 / p_0'A p_0, x_1 = x0 + alpha_1 p_0, r_1 = r_0 - alpha_1 A p_0."""
    b = np.asarray(b, dtype=np.longdouble)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.longdouble)
    r = b - csr_apply_ld(values, col, rowp, x)
    ap = csr_apply_ld(values, col, rowp, r)
    alpha = np.sum(r * r) / np.sum(r * ap)
    x1 = x + alpha * r
    r1 = r - alpha * ap
    return x1, np.sqrt(np.sum(r1 * r1))


def rel_ld(a, want):
    """Relative L2 distance of a from a long-double reference, in long double."""
    a = np.asarray(a, dtype=np.longdouble).ravel()
    want = np.asarray(want, dtype=np.longdouble).ravel()
    return float(np.sqrt(np.sum((a - want) ** 2)) / max(np.sqrt(np.sum(want * want)), np.longdouble(1e-300)))


# ---- systems --------------------------------------------------------------------------------------------------------
class Problem:
    """One matrix as the oracle holds it (compressed CSR in, the reference's slack layout inside)."""

    def __init__(self, orc, values, col, rowp):
        self.v, self.c, self.r = values, col, rowp
        self.n = len(rowp) - 1
        self.om = orc.from_csr(values, col, rowp)
        self._inv = None

    def apply(self, v):
        return self.om.apply_to_vector(v)

    @property
    def inv(self):
        if self._inv is None:
            self._inv = jacobi_inverse(self.v, self.c, self.r)
        return self._inv

    def cg(self, b, epsilon, max_iteration, init=None):
        return conjugate_gradient(self.apply, b, epsilon, max_iteration, init)

    def pcg(self, b, epsilon, max_iteration):
        return conjugate_gradient_jacobi(self.apply, self.inv, b, epsilon, max_iteration)

    def first_iteration_ld(self, b, x0=None):
        return first_iteration_ld(self.v, self.c, self.r, b, x0)


def random_spd_csr(n, seed, max_out=20, band=5000):
    """Compressed CSR of a random symmetric, strictly diagonally dominant matrix (so positive definite): row i couples to
    a few rows within `band` after it (mostly 0-3, now and then up to max_out - 1) and to those that couple to it, so
    the stored row lengths run from 1 to about 2 * max_out.  Off-diagonals -U(0.1, 1), diagonal their |sum| + U(0.5, 2);
    columns ascending within a row."""
    g = np.random.Generator(np.random.MT19937(seed))
    out_deg = (g.random(n) ** 3 * max_out).astype(np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), out_deg)
    dst = src + g.integers(1, band + 1, len(src))
    keep = dst < n
    key = np.unique(src[keep] * n + dst[keep])
    src, dst = key // n, key % n
    w = -g.uniform(0.1, 1.0, len(src))
    diag = np.bincount(src, -w, n) + np.bincount(dst, -w, n) + g.uniform(0.5, 2.0, n)
    me = np.arange(n, dtype=np.int64)
    rows = np.concatenate([src, dst, me])
    cols = np.concatenate([dst, src, me])
    vals = np.concatenate([w, w, diag])
    order = np.lexsort((cols, rows))
    rowp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowp[1:])
    return vals[order], cols[order].astype(np.int32), rowp.astype(np.int32)
