"""The cases of the multigrid soak (tools/mg_soak.py, tests/test_gpu_mg_soak.py) and their numpy models, NOT product code.
Needs numpy (scipy for the direct solve) and the model helpers of this directory: no GPU, no torch.

`cases(seed, n)` draws n case records from np.random.Generator(np.random.MT19937(seed)).  A record (Case) holds all that
rebuilds the case: the handle kind, W, H, C, the five options of capi.MG_OPTIONS, nu, the operator (or mask) class with
its seed, the per-channel scales of the right-hand side and the kind of x0.  repr(case) is one line; case_from_repr reads
it back.

What is drawn, and what is stratified.  Case i of (seed, n) has the global index j = seed * n + i, so that committed
runs of consecutive seeds and one n continue one another's strata:
  * j % 8 == 7: a "long thin" case; (j // 8) % 12 names the long side, of LONG_SIDES, and its direction; the other side
    is uniform in [1, 9100 // long side];
  * every other case has the running number t = j - j // 8.  Its (kind, precision, channels, smoother, hierarchy) is
    MODES[(t + t // 28) % 14] (the served modes of mode_walk_helpers, every kind); nu = 1 + (t // 14) % 4; the operator
    or mask class is CLASSES[(t // 14 + mode index) % len]; in even blocks of 28 values of t W = B[t % 28] and H is free,
    in odd blocks H = B[t % 28] and W is free.  A free side is B[random] or uniform [5, 200] with equal chance;
  * W H <= AREA.  If a draw exceeds it the free side is drawn again, uniform in [1, AREA // the other side]: a side that
    the strata placed stays (with two free sides, the longer one is drawn again);
  * C is 1..3 (2..3 with batched channels and with one operator per channel), the scales are of {1, 1e-6, 1e3}, x0 is
    random or zero: plain draws.

Changes a class needed so that no emitted system is one that no solver could solve (tests/test_mg_soak_cases.py):
  * `floating` is singular, so it always runs in "constant" null-space mode, and every other class in "none".  It is
    drawn only where that mode is served (sequential channels; W, H >= 2; neumann_helpers.line_served with the line
    smoother); elsewhere `benign` takes its place;
  * `fixed` needs free pixels: on a canvas with a side < 4 `zeros` takes its place, and pixel (H-1, 0) is never fixed;
  * one call has ONE epsilon, 1e-10 |b of channel 0|, so channel 0 gets the largest of the drawn scales and x0 is scaled
    with b (tests/test_gpu_mg_relative.py's construction): a channel whose b were 1e9 x channel 0's could not be reduced
    to that epsilon in float64.
  * `wide`: with weights log-uniform in [1e-3, 1e3] the model PCG needed 82..150+ iterations (both smoothers), in
    [1e-2, 1e2] up to 122; the class draws them in WIDE = [0.1, 10] (at most 47 on the committed cases);
  * `anisotropic`: wy = 1e-3 wx is what the line smoother is for, and the point-smoothed model PCG needed 62..150+
    iterations on it.  The class keeps wy = 1e-3 with the line smoother and takes wy = 0.2 with the point smoother
    (ANISOTROPY; at most 49 iterations over eight seeds).
"""
import ast
import collections
import functools
import math

import numpy as np

import constrained_helpers as ch
import line_helpers as lh
import mg_helpers as mg
import mixed_helpers as mh
import mode_walk_helpers as mw
import neumann_helpers as nh

AREA = 9100
SMALL = (1, 2, 3, 4)
TILE_SIDES = (16, 32, 64, 96, 128, 192)
DELTAS = (-1, 0, 1, 2)
B = tuple(m + d for m in TILE_SIDES for d in DELTAS) + SMALL          # 28 values; the first 24: delta fastest
LONG_SIDES = (255, 256, 257, 258, 511, 513)
SCALES = (1.0, 1e-6, 1e3)
WIDE = (0.1, 10.0)                                                   # the log-uniform range of the `wide` class
ANISOTROPY = {"line": 1e-3, "point": 0.2}                            # wy of the `anisotropic` class (wx = 1), by smoother
OPERATOR_CLASSES = ("benign", "wide", "zeros", "anisotropic", "fixed", "floating", "per_channel")
MASK_CLASSES = ("full", "ellipse", "disc", "salt", "one_pixel", "one_row", "checkerboard", "frame")
MODES = tuple((kind,) + m for kind in mw.KINDS for m in mw.served_modes(kind))   # (kind, precision, channels, smoother, hierarchy)

Case = collections.namedtuple("Case", "kind W H C hierarchy precision channels smoother nullspace nu op op_seed scales x0")

# the runs tests/test_mg_soak_cases.py and tests/test_gpu_mg_soak.py go through, and every case that ever failed
COMMITTED = [(1, 64), (2, 64)]
# The six below failed check C in the first long run (tools/mg_soak.py 2000 7, NOTES R35.1): the structured operator, on
# which the model, with numpy's sums, stopped an iteration after the device.  The model's fault: see pcg_device_order.
REGRESSIONS = [
    "Case(kind='structured', W=255, H=7, C=3, hierarchy='galerkin', precision='f64', channels='sequential', smoother='point', nullspace='none', nu=3, op='S', op_seed=310952281, scales=(1000.0, 1e-06, 1e-06), x0='random')",
    "Case(kind='structured', W=66, H=135, C=2, hierarchy='galerkin', precision='f64', channels='batched', smoother='point', nullspace='none', nu=1, op='S', op_seed=1469354371, scales=(1.0, 1e-06), x0='random')",
    "Case(kind='structured', W=65, H=131, C=1, hierarchy='galerkin', precision='f32', channels='sequential', smoother='point', nullspace='none', nu=1, op='S', op_seed=1513024808, scales=(1.0,), x0='zero')",
    "Case(kind='structured', W=111, H=63, C=3, hierarchy='galerkin', precision='f64', channels='batched', smoother='point', nullspace='none', nu=3, op='S', op_seed=729062319, scales=(1000.0, 1.0, 1000.0), x0='random')",
    "Case(kind='structured', W=33, H=96, C=2, hierarchy='galerkin', precision='f32', channels='sequential', smoother='point', nullspace='none', nu=3, op='S', op_seed=1779342943, scales=(1.0, 1e-06), x0='random')",
    "Case(kind='structured', W=15, H=130, C=3, hierarchy='galerkin', precision='f64', channels='sequential', smoother='point', nullspace='none', nu=4, op='S', op_seed=85000354, scales=(1000.0, 1e-06, 1000.0), x0='random')",
]


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


def case_from_repr(line):
    call = ast.parse(line.strip(), mode="eval").body
    if not (isinstance(call, ast.Call) and getattr(call.func, "id", None) == "Case" and not call.args):
        raise ValueError(f"not the repr of a Case: {line!r}")
    return Case(**{k.arg: ast.literal_eval(k.value) for k in call.keywords})


def mode_of(case):
    return case.kind, case.precision, case.channels, case.smoother, case.hierarchy


def is_long_thin(case):
    return max(case.W, case.H) in LONG_SIDES


# ---- the generator -----------------------------------------------------------------------------------------------------
def _free_side(g):
    return int(B[g.integers(len(B))]) if g.integers(2) else int(g.integers(5, 201))


def _shape(g, j):
    if j % 8 == 7:
        k = (j // 8) % (2 * len(LONG_SIDES))
        long_side = LONG_SIDES[k % len(LONG_SIDES)]
        other = int(g.integers(1, AREA // long_side + 1))
        return (long_side, other) if k < len(LONG_SIDES) else (other, long_side)
    t = j - j // 8
    placed = B[t % 28]
    free = _free_side(g)
    if placed * free > AREA:
        free = int(g.integers(1, AREA // placed + 1))
    return (placed, free) if (t // 28) % 2 == 0 else (free, placed)


def _class(kind, mode_index, t, W, H, channels, smoother):
    if kind == "structured":
        return "S"
    if kind == "mask":
        return MASK_CLASSES[(t // 14 + mode_index) % len(MASK_CLASSES)]
    op = OPERATOR_CLASSES[(t // 14 + mode_index) % len(OPERATOR_CLASSES)]
    if op == "floating" and not (channels == "sequential" and W >= 2 and H >= 2 and (smoother == "point" or nh.line_served(W, H))):
        op = "benign"
    if op == "fixed" and min(W, H) < 4:
        op = "zeros"
    return op


def cases(seed, n):
    g = rng(seed)
    out = []
    for i in range(n):
        j = seed * n + i
        t = j - j // 8
        mode_index = (t + t // 28) % len(MODES)
        kind, precision, channels, smoother, hierarchy = MODES[mode_index]
        W, H = _shape(g, j)
        op = _class(kind, mode_index, t, W, H, channels, smoother)
        C = int(g.integers(2, 4)) if channels == "batched" or op == "per_channel" else int(g.integers(1, 4))
        scales = sorted((SCALES[g.integers(3)] for _ in range(C)), reverse=True)
        scales = [scales[0]] + [scales[1 + k] for k in g.permutation(C - 1)]
        out.append(Case(kind=kind, W=W, H=H, C=C, hierarchy=hierarchy, precision=precision, channels=channels, smoother=smoother,
                        nullspace="constant" if op == "floating" else "none", nu=1 + (t // 14) % 4, op=op,
                        op_seed=int(g.integers(1 << 31)), scales=tuple(float(s) for s in scales),
                        x0=("random", "zero")[g.integers(2)]))
    return out


def committed_cases():
    return [c for seed, n in COMMITTED for c in cases(seed, n)]


# ---- the operators -----------------------------------------------------------------------------------------------------
def dead_block(W, H):
    """The block of dead pixels of the `zeros` class: 5 x 5 (less on a canvas without room) across x = 62..66,
    y = 30..34 when it fits, across the canvas centre otherwise."""
    bw, bh = min(5, max(W - 2, 0)), min(5, max(H - 2, 0))
    if not (bw and bh):
        return np.zeros((H, W), bool)
    x0, y0 = (62, 30) if W >= 68 and H >= 36 else (W // 2 - bw // 2, H // 2 - bh // 2)
    block = np.zeros((H, W), bool)
    block[y0:y0 + bh, x0:x0 + bw] = True
    return block


def fixed_ten(W, H, seed):
    """The `ten` set of tests/test_gpu_adjoint.py::fixed_set, with one pixel kept free."""
    m = rng(seed).uniform(size=(H, W)) < 0.1
    m[0, : max(1, W // 3)] = True
    m[H // 2:, W - 1] = True
    m[H // 2, W // 4: W // 4 + 3] = True
    m[H - 1, 0] = False
    return m.astype(np.uint8)


def _zeros(g, W, H):
    wx, wy = (g.uniform(0.5, 2.0, (H, W)) for _ in range(2))
    wx[g.uniform(size=(H, W)) < 0.1] = 0.0
    wy[g.uniform(size=(H, W)) < 0.1] = 0.0
    lam = g.uniform(1e-3, 0.3, (H, W))
    block = dead_block(W, H)
    lam[block] = 0.0
    wx[block] = 0.0
    wy[block] = 0.0
    wx[:, :-1][block[:, 1:]] = 0.0
    wy[:-1, :][block[1:, :]] = 0.0
    return wx, wy, lam


def weighted_operator(op, W, H, seed, smoother="point"):
    """(wx, wy, lam, fixed or None) of one operator of class `op` (not per_channel), float32."""
    g = rng(seed)
    fixed = None
    if op == "benign":
        wx, wy = (g.uniform(0.5, 2.0, (H, W)) for _ in range(2))
        lam = np.full((H, W), 1e-2)
    elif op == "wide":
        wx, wy = (np.exp(g.uniform(math.log(WIDE[0]), math.log(WIDE[1]), (H, W))) for _ in range(2))
        lam = g.uniform(1e-3, 0.3, (H, W))
    elif op in ("zeros", "fixed"):
        wx, wy, lam = _zeros(g, W, H)
        if op == "fixed":
            fixed = fixed_ten(W, H, seed + 1)
    elif op == "anisotropic":
        wx, wy, lam = np.full((H, W), 1.0), np.full((H, W), ANISOTROPY[smoother]), np.full((H, W), 1e-3)
    elif op == "floating":
        wx, wy = (g.uniform(0.5, 2.0, (H, W)) for _ in range(2))
        lam = np.zeros((H, W))
    else:
        raise ValueError(op)
    return wx.astype(np.float32), wy.astype(np.float32), lam.astype(np.float32), fixed


def mask_of(op, W, H, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    if op == "full":
        m = np.ones((H, W), bool)
    elif op == "ellipse":
        m = mh.ellipse_fixed(W, H) == 0
    elif op == "disc":
        from coursecomputationalphotography_amd import synth    # (numpy only)
        m = synth.disc_mask(W, H, seed=seed) != 0
    elif op == "salt":
        m = rng(seed).uniform(size=(H, W)) < 0.6
    elif op == "one_pixel":
        m = (xx == min(W - 1, 64)) & (yy == min(H - 1, 32))          # the first pixel of a second tile, where there is one
    elif op == "one_row":
        m = (yy == H // 2) & ((xx >= 3) | (W < 8)) & ((xx < W - 3) | (W < 8))
    elif op == "checkerboard":
        m = ((xx + yy) & 1) == 0
    elif op == "frame":
        m = (xx == 0) | (yy == 0) | (xx == W - 1) | (yy == H - 1)
    else:
        raise ValueError(op)
    if not m.any():
        m[H // 2, W // 2] = True
    return m.astype(np.uint8)


def operators(case, which=0):
    """The operator of every channel: a list of C entries (the same object C times for a shared operator).  weighted:
    (wx, wy, lam, fixed); mask: the mask; structured: None.  which = 1: the second operator of the class (the refresh)."""
    seed = case.op_seed + 7919 * which
    if case.kind == "structured":
        return [None] * case.C
    if case.kind == "mask":
        return [mask_of(case.op, case.W, case.H, case.op_seed)] * case.C      # (a mask is not refreshed)
    if case.op == "per_channel":
        g = rng(seed)
        return [weighted_operator(("benign", "zeros")[g.integers(2)], case.W, case.H, seed + 1 + c) for c in range(case.C)]
    op = weighted_operator(case.op, case.W, case.H, seed, case.smoother)
    if which == 1:                                                    # the fixed set and the dead pixels stay: values only
        op = op[:3] + (weighted_operator(case.op, case.W, case.H, case.op_seed)[3],)
        if case.op == "anisotropic":                                  # (the class has no random part: twice the operator)
            op = tuple(2.0 * a for a in op[:3]) + (None,)
    return [op] * case.C


# ---- the models --------------------------------------------------------------------------------------------------------
class Built:
    """The numpy side of one case: levels[c], b[c], x0[c], vb[c] (the right-hand side of the V-cycle check), eps."""


def _levels(case, op):
    if case.kind == "weighted":
        wx, wy, lam, fixed = op
        return ch.hierarchy(case.W, case.H, wx, wy, lam, fixed, case.hierarchy)
    return mg.hierarchy(case.W, case.H, op)


def build(case, which=0):
    out = Built()
    out.case, out.ops = case, operators(case, which)
    out.cs = 1.0 if case.kind == "weighted" and case.hierarchy == "rescaled" else 2.0
    shared = {}
    out.levels = []
    for op in out.ops:
        if id(op) not in shared:
            shared[id(op)] = _levels(case, op)
        out.levels.append(shared[id(op)])
    g = rng(case.op_seed + 104729)
    H, W = case.H, case.W
    out.b, out.x0, out.vb = [], [], []
    for c in range(case.C):
        A = out.levels[c][0]
        xstar = np.where(A.live, g.uniform(0.0, 255.0, (H, W)), 0.0)
        b = A.apply(xstar)
        if case.op == "floating":
            b = b + 1e-3
        out.b.append(b * case.scales[c])
        x0 = g.uniform(0.0, 255.0, (H, W)) * case.scales[c]
        inside = A.live if case.kind == "mask" else np.ones((H, W), bool)
        out.x0.append(np.where(inside, x0, 0.0) if case.x0 == "random" else np.zeros((H, W)))
        if case.nullspace == "constant":                              # integers: sums with the same bits in any order
            vb = g.integers(-50, 51, (H, W)).astype(np.float64)
            vb[0, 0] += 3.0 - (vb.sum() % 2)
        else:
            vb = np.where(A.live, g.uniform(-60.0, 60.0, (H, W)), 0.0)
        out.vb.append(vb)
    out.eps = 1e-10 * float(np.linalg.norm(out.b[0]))
    return out


def preconditioner(built, c):
    """r -> z: one V-cycle of the model of the case's mode on channel c's operator."""
    case, levels, cs = built.case, built.levels[c], built.cs
    if case.smoother == "line":
        return lambda r: lh.vcycle(levels, r, case.nu, cs)
    if case.precision == "f32":
        levels32 = mh.narrow(levels)
        return lambda r: mh.vcycle(levels32, r, case.nu, cs)
    if case.kind == "weighted":
        return lambda r: ch.vcycle(levels, r, case.nu, case.hierarchy)
    return lambda r: mg.vcycle(levels, r, case.nu)


def model_vcycle(built, c):
    """(what mg_apply leaves in x, the unprojected z, the line model's deviation or None) on vb[c]."""
    case, b = built.case, built.vb[c]
    M = preconditioner(built, c)
    dev = None
    if case.nullspace == "constant":
        want, z, bm = nh.projected_vcycle(M, b)
        if case.smoother == "line":
            dev = lh.deviation(built.levels[c], b - bm, case.nu, built.cs)[0]
        return want, z, dev
    if case.smoother == "line":
        dev, z = lh.deviation(built.levels[c], b, case.nu, built.cs)
        return z, z, dev
    z = M(b)
    return z, z, None


# ---- the PCG loop with its sums in the device's order ------------------------------------------------------------------
# Which iteration meets the epsilon is decided by the rounding of the loop's three sums, and on a nearly singular operator
# (a structured handle's: lambda = 1 at one pixel) one iteration is a factor 10..100 in the distance from the solution.  So
# the model adds up as csrc/ccp_cg.hpp and k_mg_apply (csrc/ccp_grid_mg.hpp) do, on a one-block handle:
#   * the colour-split layout: cell (x, y) at ((2 y + ((x + y) & 1)) pitch + (x >> 1), pitch = ceil(W / 2) rounded up to
#     a multiple of 16, n = 2 H pitch doubles, pads 0;
#   * a wide pass (r'r of init and update, r'z): min(2048, ceil(n / 256)) blocks of 256 threads, thread t of block k adds
#     its elements k 256 + t, + blocks 256, ... in turn; p'Ap: block (bx, by, c) of k_mg_apply's grid (agx, gy, 2), thread
#     t owns half-column bx 256 + t of colour c in rows by, by + gy, ...; the partial sum of block (bx, by, c) is stored
#     at (c gy + by) agx + bx;
#   * block_sum: wave_sum's shuffle tree (offsets 32, 16, .., 1) in each of the four waves, then the waves in turn;
#   * reduce_partials: thread t adds partial[t], partial[t + 256], ... in turn, then block_sum.
# Products are rounded before they are added (the library is built without contraction).  Batched channels and the f32
# V-cycle run the same sums per channel.  "constant" null-space mode has sums of its own (csrc/ccp_grid_mgn.hpp) and keeps
# neumann_helpers.pcg.
K_BLOCK, K_WAVE = 256, 64


def _block_sums(v):
    """block_sum of every row of v (.., 256): the value thread 0 holds."""
    w = v.reshape(v.shape[:-1] + (K_BLOCK // K_WAVE, K_WAVE))
    off = K_WAVE // 2
    while off:
        w = w[..., :off] + w[..., off:2 * off]
        off //= 2
    w = w[..., 0]
    total = np.zeros(w.shape[:-1])
    for k in range(K_BLOCK // K_WAVE):
        total = total + w[..., k]
    return total


def _strided(v, lanes):
    """Lane t adds v[t], v[t + lanes], ... in turn, from 0.0: (lanes,)."""
    m = -(-len(v) // lanes)
    a = np.zeros(m * lanes)
    a[:len(v)] = v
    a = a.reshape(m, lanes)
    acc = np.zeros(lanes)
    for k in range(m):
        acc = acc + a[k]
    return acc


def _reduce_partials(partial):
    return float(_block_sums(_strided(partial, K_BLOCK)))


class DeviceSums:
    """The two sums of the PCG loop on a W x H one-block handle, H x W arrays in, a float out."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.pitch = ((W + 1) // 2 + 15) // 16 * 16
        self.n = 2 * H * self.pitch
        yy, xx = np.mgrid[0:H, 0:W]
        self.at = ((2 * yy + ((xx + yy) & 1)) * self.pitch + (xx >> 1)).ravel()
        self.blocks = max(1, min(2048, -(-self.n // K_BLOCK)))
        self.agx = -(-((W + 1) // 2) // K_BLOCK)
        self.gy = max(1, min(H, 1024 // self.agx))

    def flat(self, a):
        out = np.zeros(self.n)
        out[self.at] = a.ravel()
        return out

    def wide(self, a, b):
        """k_cg_dot / the r'r of k_cg_init and k_cg_update, then reduce_partials."""
        acc = _strided(self.flat(a) * self.flat(b), self.blocks * K_BLOCK)
        return _reduce_partials(_block_sums(acc.reshape(self.blocks, K_BLOCK)))

    def product(self, p, ap):
        """The p'Ap of k_mg_apply, then reduce_partials."""
        v = (self.flat(p) * self.flat(ap)).reshape(self.H, 2, self.pitch).transpose(1, 0, 2)      # colour, row, half-column
        cols = np.zeros((2, self.H, self.agx * K_BLOCK))
        cols[:, :, :min(self.pitch, self.agx * K_BLOCK)] = v[:, :, :self.agx * K_BLOCK]
        acc = np.zeros((2, self.gy, self.agx * K_BLOCK))
        for y in range(self.H):                                       # row y goes to block row y % gy, in turn
            acc[:, y % self.gy] = acc[:, y % self.gy] + cols[:, y]
        partial = _block_sums(acc.reshape(2, self.gy, self.agx, K_BLOCK))                         # [(c gy + by) agx + bx]
        return _reduce_partials(partial.ravel())


def pcg_device_order(A, M, b, epsilon, max_iteration, x0):
    """mg_helpers.pcg's loop with the device's sums: (x, iterations, converged, last sqrt(r'r))."""
    sums = DeviceSums(b.shape[1], b.shape[0])
    x = np.array(x0, dtype=np.float64)
    r = b - A.apply(x)
    norm = math.sqrt(sums.wide(r, r))
    if norm < epsilon:
        return x, 0, True, norm
    z = M(r)
    rz = sums.wide(r, z)
    p = z.copy()
    cnt = 0
    while cnt < max_iteration:
        ap = A.apply(p)
        alpha = rz / sums.product(p, ap)
        x = x + alpha * p
        r = r + (-alpha) * ap
        norm = math.sqrt(sums.wide(r, r))
        if norm < epsilon:
            return x, cnt, True, norm
        z = M(r)
        rz_new = sums.wide(r, z)
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        cnt += 1
    return x, cnt, False, norm


def model_pcg(built, c, cap=60):
    """(x, iterations, converged, last sqrt(r'r)) of the model PCG of the case's mode at the call's epsilon."""
    M = preconditioner(built, c)
    if built.case.nullspace == "constant":
        return nh.pcg(built.levels[c][0], M, built.b[c], built.eps, cap, built.x0[c])[:4]
    return pcg_device_order(built.levels[c][0], M, built.b[c], built.eps, cap, built.x0[c])


# ---- the direct solve: a matrix from the header's formulas, not from the model's level 0 ------------------------------------
def matrix(case, op):
    """(A as scipy csr over the raster-ordered pixels, the solved pixels: the live free ones)."""
    import scipy.sparse as sp
    W, H = case.W, case.H
    n = W * H
    idx = np.arange(n).reshape(H, W)
    if case.kind == "mask":
        inside = (np.asarray(op) != 0)
        wx = (inside[:, :-1] & inside[:, 1:]).astype(np.float64)
        wy = (inside[:-1, :] & inside[1:, :]).astype(np.float64)
        diag = np.where(inside, 4.0, 0.0).ravel()                     # Dirichlet: a neighbour outside the region is 0
        free = inside.ravel()
    else:
        if case.kind == "structured":                                 # SolveChannel's matrix
            yy, xx = np.mgrid[0:H, 0:W]
            cell = ((xx < W - 1) & (yy < H - 1)).astype(np.float64)
            wxf, wyf, lam, fixed = cell, cell, np.zeros((H, W)), None
            lam[0, 0] = 1.0
        else:
            wxf, wyf, lam, fixed = (None if a is None else np.asarray(a, dtype=np.float64) for a in op)
        wx, wy = wxf[:, :-1], wyf[:-1, :]
        diag = lam.copy()
        diag[:, :-1] += wx
        diag[:, 1:] += wx
        diag[:-1, :] += wy
        diag[1:, :] += wy
        diag = diag.ravel()
        free = np.ones(n, bool) if fixed is None else (np.asarray(fixed) == 0).ravel()
    a, b_ = idx[:, :-1].ravel(), idx[:, 1:].ravel()
    c, d = idx[:-1, :].ravel(), idx[1:, :].ravel()
    rows = np.concatenate([np.arange(n), a, b_, c, d])
    cols = np.concatenate([np.arange(n), b_, a, d, c])
    vals = np.concatenate([diag, -wx.ravel(), -wx.ravel(), -wy.ravel(), -wy.ravel()])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    return A, free & (diag != 0)


def direct(built, c):
    """(x of the direct solve on the solved pixels, 0 elsewhere; the solved pixels as an H x W mask).  A floating system:
    the mean-free solution of the bordered system."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    case = built.case
    A, solved = matrix(case, built.ops[c])
    keep = np.flatnonzero(solved)
    b = built.b[c].ravel()[keep]
    Ak = A[keep][:, keep].tocsc()
    if case.nullspace == "constant":
        one = sp.csc_matrix(np.ones((len(keep), 1)))
        K = sp.bmat([[Ak, one], [one.T, None]], format="csc")
        sol = sla.spsolve(K, np.concatenate([b, [0.0]]))[:-1]
    else:
        sol = sla.spsolve(Ak, b) if len(keep) > 1 else b / Ak.toarray().ravel()
    x = np.zeros(case.W * case.H)
    x[keep] = sol
    return x.reshape(case.H, case.W), solved.reshape(case.H, case.W)


def distance(built, c, x, ref, solved):
    """max |x - ref| over the solved pixels; a floating system: of the mean-free parts."""
    if built.case.nullspace == "constant":
        x = x - nh.mean(x)
        ref = ref - nh.mean(ref)
    return float(np.max(np.abs(np.where(solved, x - ref, 0.0))))


@functools.lru_cache(maxsize=256)
def cached(case, which=0):
    return build(case, which)
