"""Row blocks with ghost rows, swept block by block with the halos exchanged by hand (test infrastructure).

RowBlocks holds one handle per [cuts[i], cuts[i + 1]) and does what a multi-rank run does between two halo exchanges:
every block sweeps n times on its own (2 n <= ghost: validity recedes one row per half-sweep from a stale edge), the owned
rows are gathered into the full image, every block's local rows (ghosts included) are written back and the handle is told
that its halo is fresh.  run_intervals drives it over a list of sweep counts and returns the full image after each.
The handle is anything with set_b, fill_x, set_x, get_x_owned, sweep, halo_refreshed, first_local_row and local_rows:
capi.Grid by default, NumpyBlock (a plain numpy red-black update) in tests/test_rowblock_sweep_helpers.py, which shows
without a GPU that the exchange arithmetic is right.

Also here: CASES, the row-block shapes of tests/test_gpu_rowblock_depth8.py, and the reader of a CCP_GS_TRACE_FILE
(trace_passes, wide_passes, wide_strips) that tests/test_gpu_wide_segments.py shares."""
import numpy as np

KERNEL_WIDE = 3                           # the kernel id k_fused_sweep_wide writes into its trace records
TRACE_MAGIC = 0x43435054524143
T = 8

# name: (W, H, C, cuts, ghost, chunk rows, sweeps per refresh interval, a block has an odd first local row)
CASES = {
    "A": (673, 401, 1, [0, 133, 268, 401], 64, 32, [32, 32], True),         # first local rows 0, 69, 204; 4 depth-8 passes
    "B": (673, 401, 3, [0, 133, 268, 401], 32, 32, [16, 16, 16], True),     # 0, 101, 236; three channels, 2 passes
    "C": (449, 300, 1, [0, 81, 300], 32, 16, [16, 16], True),               # 0, 49; a whole and a partial wide strip, both blocks at an image end
    "D": (898, 523, 2, [0, 111, 222, 305, 523], 64, 48, [32, 32], True),    # 0, 47, 158, 241; partial wide strip at the right
    "E": (673, 401, 1, [0, 191, 211, 401], 64, 32, [32, 32], True),         # 0, 127, 147; a 20-row block: range under the halo
    "F": (1001, 333, 1, [0, 109, 222, 333], 64, 32, [27, 32, 5], True),     # 0, 45, 158; mixed depths, last interval shallow
}


def first_local_rows(cuts, ghost):
    """image row of local row 0 of every block (ccp_grid_create: the ghost is clipped at the image)"""
    return [cuts[i] - min(ghost, cuts[i]) for i in range(len(cuts) - 1)]


def default_factory(W, H, C, row_begin, row_count, ghost):
    from coursecomputationalphotography_amd import capi
    return capi.Grid(W, H, C, row_begin, row_count, ghost)


class RowBlocks:
    """bs: per channel, the right-hand side of the whole image (H * W values); tiling: (max depth, chunk rows) or None"""

    def __init__(self, W, H, C, cuts, ghost, bs, tiling=None, factory=None):
        if cuts[0] != 0 or cuts[-1] != H or any(b <= a for a, b in zip(cuts, cuts[1:])):
            raise ValueError("cuts must rise from 0 to H")
        self.W, self.H, self.C, self.cuts, self.ghost = W, H, C, list(cuts), ghost
        factory = factory or default_factory
        self.blocks = []
        for i in range(len(cuts) - 1):
            g = factory(W, H, C, cuts[i], cuts[i + 1] - cuts[i], ghost)
            self.blocks.append(g)                       # (before anything can raise: close() reaches it)
            lo = g.first_local_row
            for ch in range(C):
                g.set_b(np.asarray(bs[ch], dtype=np.float64).reshape(H, W)[lo:lo + g.local_rows], ch)
            g.fill_x(1.0)
            if tiling:
                g.set_tiling(*tiling)

    def sweep(self, n):
        """n sweeps of every block on the halo it has; refuses a count the ghosts cannot carry"""
        if len(self.blocks) > 1 and 2 * n > self.ghost:
            raise ValueError(f"{n} sweeps need {2 * n} ghost rows, the blocks have {self.ghost}")
        for g in self.blocks:
            g.sweep(n)

    def gather(self):
        """per channel, the full image from the owned rows of every block"""
        return [np.concatenate([g.get_x_owned(ch) for g in self.blocks]) for ch in range(self.C)]

    def refresh(self, full):
        """every block's local rows, ghosts included, from the full image"""
        for g in self.blocks:
            lo = g.first_local_row
            for ch in range(self.C):
                g.set_x(full[ch][lo:lo + g.local_rows], ch)
            g.halo_refreshed()

    def close(self):
        for g in self.blocks:
            if hasattr(g, "close"):
                g.close()
        self.blocks = []


def run_intervals(W, H, C, cuts, ghost, sweeps, bs, tiling=None, factory=None):
    """Per refresh interval, per channel: the full H x W image after that interval's sweeps."""
    rb = RowBlocks(W, H, C, cuts, ghost, bs, tiling, factory)
    try:
        out = []
        for n in sweeps:
            rb.sweep(n)
            full = rb.gather()
            out.append(full)
            rb.refresh(full)
        return out
    finally:
        rb.close()


# ---- the tiling of a depth-8 pass over a row block, restated from launch_fused / fused_tile_counts ----------------------
def block_interior(H, y0, st_lo, st_hi, R):
    """(nb_top, nb_bot, wide_y0, wide_y1): the border chunk rows at the image's top and bottom, and the local rows of the
    chunks between them (the wide interior), of a depth-8 pass that stores local rows [st_lo, st_hi) of a block whose
    local row 0 is image row y0; None when the pass has no ordinary chunk"""
    HS, short = 2 * T, 2 * T + 16
    rows = st_hi - st_lo
    cut = rows > 2 * short + R // 2 and R > short
    first = short if (cut and y0 + st_lo - HS <= 0) else 0
    last = short if (cut and y0 + st_hi + HS >= H - 1) else 0
    n_chunks = -(-(rows - first - last) // R) + (first > 0) + (last > 0)

    def chunk(c):
        if first and c == 0:
            return st_lo, st_lo + first
        if last and c == n_chunks - 1:
            return st_hi - last, st_hi
        ra = st_lo + first + (c - (1 if first else 0)) * R
        return ra, min(ra + R, st_hi - last)

    nb_top = 0
    while nb_top < n_chunks and y0 + chunk(nb_top)[0] - HS <= 0:
        nb_top += 1
    nb_bot = 0
    while nb_top + nb_bot < n_chunks and y0 + chunk(n_chunks - 1 - nb_bot)[1] + HS >= H - 1:
        nb_bot += 1
    if nb_top + nb_bot >= n_chunks:
        return None
    return nb_top, nb_bot, chunk(nb_top)[0], chunk(n_chunks - nb_bot - 1)[1]


def depth8_passes(H, cuts, ghost, R, n_passes):
    """per block, per depth-8 pass since the last refresh: (st_lo, st_hi, block_interior(...)); the stored rows lose 16
    per pass on every side that is a stale edge, down to the owned rows"""
    out = []
    for i, y0 in enumerate(first_local_rows(cuts, ghost)):
        top, bottom = cuts[i] - y0, min(ghost, H - cuts[i + 1])
        local = top + cuts[i + 1] - cuts[i] + bottom
        passes = []
        for k in range(n_passes):
            st_lo = min(2 * T * (k + 1), top) if y0 > 0 else 0
            st_hi = local - (min(2 * T * (k + 1), bottom) if y0 + local < H else 0)
            passes.append((st_lo, st_hi, block_interior(H, y0, st_lo, st_hi, R)))
        out.append(passes)
    return out


# ---- a numpy stand-in for the handle ------------------------------------------------------------------------------
class NumpyBlock:
    """Local rows of a red-black, radius-1 update: x = (((up + left) + right) + down + b) * (1 / neighbours inside the image),
    red ((column + image row) even) first.  A neighbour outside the IMAGE does not count (the update's edge rule); a
    neighbour outside the BLOCK counts and reads 0, so the rows next to a stale edge go wrong one row per half-sweep,
    as they do in the real handle."""

    def __init__(self, W, H, C, row_begin, row_count, ghost):
        top = min(ghost, row_begin)
        bottom = min(ghost, H - row_begin - row_count)
        self.W, self.H, self.C = W, H, C
        self.row_begin, self.row_count = row_begin, row_count
        self.first_local_row = row_begin - top
        self.local_rows = top + row_count + bottom
        self.stale = (self.first_local_row > 0, self.first_local_row + self.local_rows < H)
        self.ghost = ghost
        self.half_sweeps = 0
        self.b = np.zeros((C, self.local_rows, W))
        self.padded = np.zeros((C, self.local_rows + 2, W + 2))     # zero outside the block and outside the image
        self.x = self.padded[:, 1:-1, 1:-1]                        # (a view)
        ys = np.arange(self.first_local_row, self.first_local_row + self.local_rows)[:, None]
        xs = np.arange(W)[None, :]
        count = ((ys > 0).astype(np.float64) + (ys < H - 1)) + ((xs > 0).astype(np.float64) + (xs < W - 1))
        self.inv = 1.0 / np.maximum(count, 1.0)         # (a 1 x 1 image)

    def set_b(self, rows, channel=0):
        self.b[channel] = np.asarray(rows, dtype=np.float64).reshape(self.local_rows, self.W)

    def set_x(self, rows, channel=0):
        self.x[channel] = np.asarray(rows, dtype=np.float64).reshape(self.local_rows, self.W)

    def fill_x(self, value=1.0):
        self.x[:] = value

    def get_x_owned(self, channel=0):
        lo = self.row_begin - self.first_local_row
        return self.x[channel, lo:lo + self.row_count].copy()

    def halo_refreshed(self):
        self.half_sweeps = 0

    def sweep(self, iterations):
        p, R, W = self.padded, self.local_rows, self.W
        for _ in range(iterations):
            for colour in (0, 1):                       # red: (column + image row) even
                if any(self.stale):
                    assert self.half_sweeps < self.ghost, "ghosts exhausted: refresh the halo first"
                    self.half_sweeps += 1
                for a in (0, 1):                        # local rows a, a + 2, ...: their pixels of this colour are columns c, c + 2, ...
                    c = (colour + self.first_local_row + a) & 1
                    rows, cols = slice(1 + a, R + 1, 2), slice(1 + c, W + 1, 2)
                    t = (p[:, a:R:2, cols] + p[:, rows, c:W:2]) + p[:, rows, 2 + c:W + 2:2]
                    t += p[:, 2 + a:R + 2:2, cols]
                    t += self.b[:, a::2, c::2]
                    t *= self.inv[a::2, c::2]
                    p[:, rows, cols] = t


# ---- the per-wave trace of the blocked passes (CCP_GS_TRACE_FILE) ---------------------------------------------------
def trace_passes(path):
    """per recorded pass: (depth, [(kernel id, chunk or segment, strip, channel) of every wave that ran])"""
    raw = np.fromfile(path, dtype=np.uint64)
    out, i = [], 0
    while i < raw.size:
        assert raw[i] == TRACE_MAGIC
        n = int(raw[i + 6])
        rec = raw[i + 8:i + 8 + n].reshape(-1, 4)
        rec = rec[rec[:, 1] != 0]
        out.append((int(raw[i + 1]),
                    [((int(t) >> 40) & 0xff, int(t) & 0xffff, (int(t) >> 16) & 0xffff, (int(t) >> 32) & 0xff) for t in rec[:, 3]]))
        i += 8 + n
    return out


def wide_passes(path):
    """per recorded pass that ran the wide kernel: the (segment, strip, channel) of its records"""
    out = []
    for _, waves in trace_passes(path):
        tiles = [w[1:] for w in waves if w[0] == KERNEL_WIDE]
        if tiles:
            out.append(tiles)
    return out


def wide_strips(W):
    """wide strips of a depth-8 pass over W columns, restated from launch_fused_t / fused_tile_counts"""
    U, n = 128 - 4 * T, -(-W // (128 - 4 * T))
    left = 0
    while left < n and left * U - 2 * T <= 0:
        left += 1
    right = 0
    while left + right < n and (n - 1 - right) * U - 2 * T + 128 >= W - 1:
        right += 1
    return -(-((n - right) * U - left * U) // (256 - 4 * T))
