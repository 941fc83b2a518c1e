// ccp_grid_mgb.hpp — the batched mode of the multigrid-preconditioned conjugate gradient (include/ccp_gs.h,
// CCP_MG_CHANNELS_BATCHED), hand-written for gfx950: every launch of ccp_grid_mg.hpp's PCG loop serves all channels of a
// handle, and whatever does not depend on the channel -- the operator's coefficients -- is fetched once per launch.
//
// Definition.  The channels never mix, so channel ch gets, bit for bit, what the sequential kernels (k_mg_*, k_cg_*) give
// it.  The arithmetic is theirs by construction: the tail's cycle (mg_tail_body), the per-cell formulas (mg_nb_sum,
// mg_stored_update, mg_stored_residual, mg_masked_update, mg_masked_row, gs_update, apply_row), the CG passes' bodies
// (cg_*_body, cg_*_step, mg_check_step, mg_beta_step) are the functions the sequential kernels call, on a channel's slice.
// What this file adds is where the operands come from and the grouping of every partial sum, which is the sequential
// one (the same grid within a channel, block_sum, reduce_partials over the channel's slice of the partial sums).  A
// channel whose st[ch].active is 0 is skipped as a whole launch is there.
//
// Vectors.  Channel ch of a vector sits `stride` doubles after channel 0 (the handle's x and b: ch_stride; the PCG
// vectors and level 0's t likewise; a coarse level's b, z, t: the level's size).  CgState[C]; the partial sums are C
// slices `ps` doubles apart.
//
// k_mgb_tile keeps the coefficients of its (64 + 4 nu) x (32 + 4 nu) region in LDS for all channels: d, we, ws of a
// stored operator (three fp64 planes beside b and z: 40 B per cell, 115,200 B at nu = 2, 153,600 B at nu = 4 -- one
// workgroup per CU, which therefore runs 1,024 threads: mgb_tile_threads), one byte per cell otherwise (a mask byte, or
// classify's result packed).  No coefficient is read from global memory inside a half-sweep.  k_mgb_restrict and
// k_mgb_apply load the coefficients of a thread's cells into registers once and loop over up to kMgbGroup channels;
// further channel groups lie on grid z.
#pragma once

#include "ccp_grid_mg.hpp"

namespace ccp {

constexpr int kMgbGroup = 4;                                      // channels per thread of k_mgb_restrict / k_mgb_apply

// dynamic LDS of k_mgb_tile: b and z of one channel, and the region's coefficients
__host__ __device__ constexpr int mgb_tile_lds(int kind, int nu)
{
    const int cells = (kMgTileW + 4 * nu) * (kMgTileH + 4 * nu);
    return kind == kMgCoarse ? 5 * cells * (int)sizeof(double) : 2 * cells * (int)sizeof(double) + (cells + 7) / 8 * 8;
}

// Threads of a k_mgb_tile workgroup.  Which thread updates a cell does not change the cell's arithmetic (the pass has no
// sums), so the stored-operator kind, whose LDS leaves room for one workgroup per CU, runs 16 waves instead of 4.
__host__ __device__ constexpr int mgb_tile_threads(int kind) { return kind == kMgCoarse ? 1024 : kBlock; }

__device__ __forceinline__ bool mgb_any_active(const CgState *__restrict__ st, int C)
{
    if (!st) return true;
    bool any = false;
    for (int ch = 0; ch < C; ++ch) any = any || st[ch].active != 0;
    return any;
}

// classify's result in a byte: up, left, right, down in bits 0..3, the diagonal (0..5) from bit 4
__device__ __forceinline__ unsigned char mgb_pack(const Stencil &s)
{
    return (unsigned char)((int)s.up | (int)s.left << 1 | (int)s.right << 2 | (int)s.down << 3 | s.diag << 4);
}

__device__ __forceinline__ Stencil mgb_unpack(unsigned char f)
{
    Stencil s;
    s.up = f & 1;
    s.left = f & 2;
    s.right = f & 4;
    s.down = f & 8;
    s.diag = f >> 4;
    return s;
}

// ---- one level of the V-cycle ------------------------------------------------------------------------------------------
// k_mg_tile for all channels: the region's coefficients go to LDS once, then every active channel in turn is loaded,
// smoothed by the 2 nu half-sweeps and stored.  fs: the channel stride of b, z_in, z_out; es: of ec.  grid as k_mg_tile's;
// dynamic LDS mgb_tile_lds(KIND, nu) bytes.
template <int KIND, bool POST>
__global__ void __launch_bounds__(mgb_tile_threads(KIND))
k_mgb_tile(MgLevel lv, const double *__restrict__ b, const double *__restrict__ z_in, double *__restrict__ z_out, long fs, MgLevel cv,
           const double *__restrict__ ec, long es, double cs, int nu, int C, const CgState *__restrict__ st)
{
    extern __shared__ double mgb_lds[];
    constexpr int NT = mgb_tile_threads(KIND);
    if (!mgb_any_active(st, C)) return;                              // (uniform)
    const int h = 2 * nu, RW = kMgTileW + 2 * h, RH = kMgTileH + 2 * h, n = RW * RH;
    double *sb = mgb_lds, *sz = mgb_lds + n;
    double *sd = mgb_lds + 2 * n, *swe = mgb_lds + 3 * n, *sws = mgb_lds + 4 * n;   // kMgCoarse
    unsigned char *sf = reinterpret_cast<unsigned char *>(mgb_lds + 2 * n);       // kMgMasked: the mask byte; kMgSolve: mgb_pack
    const int x0 = blockIdx.x * kMgTileW - h, y0 = lv.lo + blockIdx.y * kMgTileH - h;
    for (int i = threadIdx.x; i < n; i += NT) {                      // outside the level: dead, every weight 0
        const int x = x0 + i % RW, y = y0 + i / RW;
        const bool in = x >= 0 && x < lv.W && y >= 0 && y < lv.H;
        const long at = in ? mg_at(lv.pitch, x, y) : 0;
        if (KIND == kMgCoarse) {
            sd[i] = in ? lv.d[at] : 0.0;
            swe[i] = in ? lv.we[at] : 0.0;
            sws[i] = in ? lv.ws[at] : 0.0;
        } else if (KIND == kMgMasked) {
            sf[i] = in ? lv.mask[at] : (unsigned char)0;
        } else {
            Stencil none{};
            sf[i] = mgb_pack(in ? classify(lv.g0, x, lv.y0 + y, y) : none);
        }
    }
    // (a thread reads back below only what it wrote above, until the first barrier of the channel loop)
    const int hw = RW / 2;
    for (int ch = 0; ch < C; ++ch) {
        if (st && !st[ch].active) continue;                          // (uniform)
        const double *__restrict__ bc = b + ch * fs;
        for (int i = threadIdx.x; i < n; i += NT) {
            const int x = x0 + i % RW, y = y0 + i / RW;
            double bv = 0.0, zv = 0.0;
            if (x >= 0 && x < lv.W && y >= 0 && y < lv.H) {
                const long at = mg_at(lv.pitch, x, y);
                bv = bc[at];
                if (POST) {
                    zv = z_in[ch * fs + at];
                    const bool live = KIND == kMgCoarse ? sd[i] != 0.0 : KIND == kMgMasked ? sf[i] != 0 : (sf[i] >> 4) != 0;
                    if (live) zv = zv + cs * ec[ch * es + mg_at(cv.pitch, x >> 1, ((lv.y0 + y) >> 1) - cv.y0)];
                }
            }
            sb[i] = bv;
            sz[i] = zv;
        }
        __syncthreads();
        auto half_sweep = [&](int c) {
            for (int k = threadIdx.x; k < hw * RH; k += NT) {
                const int r = k / hw, y = y0 + r;
                const int col = 2 * (k % hw) + ((c + y) & 1), x = x0 + col;
                if (x < 0 || x >= lv.W || y < 0 || y >= lv.H) continue;
                const int i = r * RW + col;
                const double xu = r > 0 ? sz[i - RW] : 0.0, xd = r + 1 < RH ? sz[i + RW] : 0.0;
                const double xl = col > 0 ? sz[i - 1] : 0.0, xr = col + 1 < RW ? sz[i + 1] : 0.0;
                const double bv = sb[i];
                double out = 0.0;
                if (KIND == kMgSolve) {
                    if (!gs_update(mgb_unpack(sf[i]), bv, xu, xl, xr, xd, out)) out = 0.0;
                } else if (KIND == kMgMasked) {
                    out = sf[i] ? mg_masked_update(bv, xu, xl, xr, xd) : 0.0;
                } else {
                    const double d = sd[i];
                    if (d != 0.0) {
                        const double s = mg_nb_sum(r > 0 ? sws[i - RW] : 0.0, xu, col > 0 ? swe[i - 1] : 0.0, xl, swe[i], xr, sws[i], xd);
                        out = mg_stored_update(bv, s, d);
                    }
                }
                sz[i] = out;
            }
            __syncthreads();
        };
        for (int s = 0; s < nu; ++s) {
            half_sweep(POST ? 1 : 0);
            half_sweep(POST ? 0 : 1);
        }
        double *__restrict__ zo = z_out + ch * fs;
        for (int i = threadIdx.x; i < kMgTileW * kMgTileH; i += NT) {
            const int col = h + i % kMgTileW, r = h + i / kMgTileW, x = x0 + col, y = y0 + r;
            if (x < lv.W && y < lv.hi) zo[mg_at(lv.pitch, x, y)] = sz[r * RW + col];
        }
        __syncthreads();                                             // the next channel's load overwrites sb, sz
    }
}

// What mg_residual and mg_row0 need of pixel (x,y) that no channel changes
// (the flags share one register: a bool apiece would cost a pair of SGPRs per flag and cell)
enum : unsigned { kMgbIn = 1, kMgbLive = 2, kMgbUp = 4, kMgbLeft = 8, kMgbRight = 16, kMgbDown = 32 };
template <int KIND>
struct MgbCell {
    unsigned f;                      // kMgbIn: inside the level's owned rows; kMgbLive: a live pixel; kMgbUp ..: that
                                     // neighbour lies inside the level; kMgSolve: mgb_pack(classify) from bit 8
    long at, au, al, ar, ad;
    double d, wn, ww, we, ws;        // kMgCoarse: the diagonal and the weights to the four neighbours
};

template <int KIND>
__device__ __forceinline__ MgbCell<KIND> mgb_cell(const MgLevel &lv, int x, int y)
{
    MgbCell<KIND> c{};
    if (!(x < lv.W && y >= lv.lo && y < lv.hi)) return c;
    const bool hu = y >= 1, hl = x >= 1, hr = x + 1 < lv.W, hd = y + 1 < lv.H;
    c.f = kMgbIn | (hu ? kMgbUp : 0u) | (hl ? kMgbLeft : 0u) | (hr ? kMgbRight : 0u) | (hd ? kMgbDown : 0u);
    c.at = mg_at(lv.pitch, x, y);
    c.au = hu ? mg_at(lv.pitch, x, y - 1) : 0;
    c.al = hl ? mg_at(lv.pitch, x - 1, y) : 0;
    c.ar = hr ? mg_at(lv.pitch, x + 1, y) : 0;
    c.ad = hd ? mg_at(lv.pitch, x, y + 1) : 0;
    bool live;
    if (KIND == kMgSolve) {
        const Stencil s = classify(lv.g0, x, lv.y0 + y, y);
        c.f |= (unsigned)mgb_pack(s) << 8;
        live = s.diag != 0;
    } else if (KIND == kMgMasked) {
        live = lv.mask[c.at] != 0;
    } else {
        c.d = lv.d[c.at];
        live = c.d != 0.0;
        c.wn = hu ? lv.ws[c.au] : 0.0;
        c.ww = hl ? lv.we[c.al] : 0.0;
        c.we = lv.we[c.at];
        c.ws = lv.ws[c.at];
    }
    if (live) c.f |= kMgbLive;
    return c;
}

// mg_row0 of one channel's z
template <int KIND>
__device__ __forceinline__ double mgb_row0(const MgbCell<KIND> &c, const double *__restrict__ z)
{
    if (KIND == kMgCoarse) {                                         // weighted_row
        if (c.d == 0.0) return 0.0;
        double a = 0.0;
        if (c.f & kMgbUp) a += -(c.wn * z[c.au]);
        if (c.f & kMgbLeft) a += -(c.ww * z[c.al]);
        a += c.d * z[c.at];
        if (c.f & kMgbRight) a += -(c.we * z[c.ar]);
        if (c.f & kMgbDown) a += -(c.ws * z[c.ad]);
        return a;
    }
    const double xi = z[c.at];
    const double xu = c.f & kMgbUp ? z[c.au] : 0.0, xl = c.f & kMgbLeft ? z[c.al] : 0.0;
    const double xr = c.f & kMgbRight ? z[c.ar] : 0.0, xd = c.f & kMgbDown ? z[c.ad] : 0.0;
    if (KIND == kMgSolve) return apply_row(mgb_unpack((unsigned char)(c.f >> 8)), xi, xu, xl, xr, xd);
    double ax = 0.0;
    if (c.f & kMgbLive) ax = mg_masked_row(xi, xu, xl, xr, xd);
    return ax;
}

// mg_residual of one channel's b and z
template <int KIND>
__device__ __forceinline__ double mgb_residual(const MgbCell<KIND> &c, const double *__restrict__ b, const double *__restrict__ z)
{
    if (!(c.f & kMgbIn) || !(c.f & kMgbLive)) return 0.0;
    if constexpr (KIND != kMgCoarse) {
        return b[c.at] - mgb_row0<KIND>(c, z);
    } else {
        const double xi = z[c.at];
        const double xu = c.f & kMgbUp ? z[c.au] : 0.0, xl = c.f & kMgbLeft ? z[c.al] : 0.0;
        const double xr = c.f & kMgbRight ? z[c.ar] : 0.0, xd = c.f & kMgbDown ? z[c.ad] : 0.0;
        return mg_stored_residual(b[c.at], c.d, xi, mg_nb_sum(c.wn, xu, c.ww, xl, c.we, xr, c.ws, xd));
    }
}

// k_mg_restrict for the channels [kMgbGroup z, kMgbGroup (z + 1)) of blockIdx.z = z.  fs: the channel stride of b and z,
// es: of bc.  grid = (ceil(Wc/kBlock), coarse rows from local row Y0, channel groups).
template <int KIND>
__global__ void __launch_bounds__(kBlock)
k_mgb_restrict(MgLevel lv, const double *__restrict__ b, const double *__restrict__ z, long fs, MgLevel cv, int Y0, double *__restrict__ bc,
               long es, int C, const CgState *__restrict__ st)
{
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = Y0 + (int)blockIdx.y;
    if (X >= cv.W) return;
    const int ch0 = blockIdx.z * kMgbGroup, ch1 = min(C, ch0 + kMgbGroup);
    bool any = !st;
    for (int ch = ch0; ch < ch1 && !any; ++ch) any = st[ch].active != 0;
    if (!any) return;
    const int x = 2 * X, y = 2 * (cv.y0 + Y) - lv.y0;
    const MgbCell<KIND> c00 = mgb_cell<KIND>(lv, x, y), c10 = mgb_cell<KIND>(lv, x + 1, y);
    const MgbCell<KIND> c01 = mgb_cell<KIND>(lv, x, y + 1), c11 = mgb_cell<KIND>(lv, x + 1, y + 1);
    const long to = mg_at(cv.pitch, X, Y);
    for (int ch = ch0; ch < ch1; ++ch) {
        if (st && !st[ch].active) continue;
        const double *__restrict__ bb = b + ch * fs, *__restrict__ zz = z + ch * fs;
        const double r00 = mgb_residual<KIND>(c00, bb, zz), r10 = mgb_residual<KIND>(c10, bb, zz);
        const double r01 = mgb_residual<KIND>(c01, bb, zz), r11 = mgb_residual<KIND>(c11, bb, zz);
        bc[ch * es + to] = (r00 + r10) + (r01 + r11);
    }
}

// k_mg_apply for the channels of group blockIdx.z >> 1, colour blockIdx.z & 1: out := A in per channel (vs: the channel
// stride of in and out).  DOT: channel ch's partial sums in its slice, partial + ch * ps, at k_mg_apply's index.
// grid = (k_mg_apply's x, its y, 2 x channel groups).
template <int KIND, bool DOT>
__global__ void __launch_bounds__(kBlock)
k_mgb_apply(MgLevel lv, const double *__restrict__ in, double *__restrict__ out, long vs, double *__restrict__ partial, long ps, int C,
            const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    const int c = blockIdx.z & 1, ch0 = (int)(blockIdx.z >> 1) * kMgbGroup;
    bool act[kMgbGroup];
    bool any = false;
#pragma unroll
    for (int q = 0; q < kMgbGroup; ++q) {
        act[q] = ch0 + q < C && (!st || st[ch0 + q].active != 0);    // (uniform)
        any = any || act[q];
    }
    if (!any) return;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    double dot[kMgbGroup];
#pragma unroll
    for (int q = 0; q < kMgbGroup; ++q) dot[q] = 0.0;
    for (int y = lv.lo + blockIdx.y; y < lv.hi; y += gridDim.y) {
        const int x = 2 * j + ((y + c) & 1);
        if (x < lv.W) {
            const MgbCell<KIND> cell = mgb_cell<KIND>(lv, x, y);
#pragma unroll
            for (int q = 0; q < kMgbGroup; ++q) {
                if (!act[q]) continue;
                const double *__restrict__ zq = in + (ch0 + q) * vs;
                const double ax = mgb_row0<KIND>(cell, zq);
                out[(ch0 + q) * vs + cell.at] = ax;
                dot[q] += zq[cell.at] * ax;
            }
        }
    }
    if (DOT) {
#pragma unroll
        for (int q = 0; q < kMgbGroup; ++q) {
            if (!act[q]) continue;
            const double t = block_sum(dot[q], scratch);
            if (threadIdx.x == 0) partial[(ch0 + q) * ps + ((long)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// ---- the tail: mg_tail_body (ccp_grid_mg.hpp), one workgroup per channel (bs, zs: the channel strides of b_top, z_top) -----
static __global__ void __launch_bounds__(kBlock)
k_mgb_tail(MgTail t, const double *__restrict__ b_top, double *__restrict__ z_top, long bs, long zs, double cs, int nu,
           const CgState *__restrict__ st)
{
    if (st && !st[blockIdx.x].active) return;
    mg_tail_body(t, b_top + blockIdx.x * bs, z_top + blockIdx.x * zs, cs, nu);
}

// ---- the vector passes: the bodies of k_cg_init, k_cg_dot, k_cg_update, k_cg_direction (ccp_cg.hpp), the channel on grid y ----
// grid = (the sequential pass's blocks, C).  Every vector has the channel stride n; partial: C slices ps apart.
static __global__ void __launch_bounds__(kBlock)
k_mgb_init(const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p, long n, double *__restrict__ partial, long ps)
{
    __shared__ double scratch[kBlock / kWave];
    const long o = (long)blockIdx.y * n;
    const double t = block_sum(cg_init_body(b, r, p, o, n), scratch);
    if (threadIdx.x == 0) partial[blockIdx.y * ps + blockIdx.x] = t;
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_dot(const double *__restrict__ a, const double *__restrict__ b, long n, double *__restrict__ partial, long ps,
          const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    const long o = (long)blockIdx.y * n;
    const double t = block_sum(cg_dot_body(a, b, o, n, st + blockIdx.y), scratch);
    if (threadIdx.x == 0) partial[blockIdx.y * ps + blockIdx.x] = t;
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_update(double *__restrict__ x, const double *__restrict__ p, double *__restrict__ r, const double *__restrict__ ap, long n,
             double *__restrict__ partial, long ps, const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    const long o = (long)blockIdx.y * n;
    const double t = block_sum(cg_update_body(x, p, r, ap, o, n, st + blockIdx.y), scratch);
    if (threadIdx.x == 0) partial[blockIdx.y * ps + blockIdx.x] = t;
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_direction(double *__restrict__ p, const double *__restrict__ z, long n, const CgState *__restrict__ st)
{
    cg_direction_body(p, z, (long)blockIdx.y * n, n, st + blockIdx.y);
}

// ---- the scalar passes: the steps of k_cg_set_rlen, k_cg_alpha, k_mg_check, k_mg_beta, one workgroup per channel ----------
static __global__ void __launch_bounds__(kBlock)
k_mgb_set_rlen(const double *__restrict__ partial, long ps, int count, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    cg_set_rlen_step(reduce_partials(partial + blockIdx.x * ps, count, scratch), st + blockIdx.x);
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_alpha(const double *__restrict__ partial, long ps, int count, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    cg_alpha_step(reduce_partials(partial + blockIdx.x * ps, count, scratch), st + blockIdx.x);
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_check(const double *__restrict__ partial, long ps, int count, double epsilon, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mg_check_step(reduce_partials(partial + blockIdx.x * ps, count, scratch), epsilon, st + blockIdx.x);
}

static __global__ void __launch_bounds__(kBlock)
k_mgb_beta(const double *__restrict__ partial, long ps, int count, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mg_beta_step(reduce_partials(partial + blockIdx.x * ps, count, scratch), st + blockIdx.x);
}

}  // namespace ccp
