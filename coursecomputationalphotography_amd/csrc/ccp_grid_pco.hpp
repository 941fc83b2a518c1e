// ccp_grid_pco.hpp — a weighted grid handle with one operator PER CHANNEL (include/ccp_gs.h,
// ccp_grid_set_weights_per_channel_device), hand-written for gfx950: the formation of all channels' planes with its
// validation, the right-hand side of every channel from its own planes, the coarsening of all channels' levels, and the
// operator-dependent passes of the batched PCG (tile, restrict, tail, product) with the channel on a grid axis.
//
// Definition.  Channel c's planes (d, we, ws, lambda, and with a fixed mask ce, cs, lambda') are what
// ccp_grid_set_weights_constrained_device forms on a one-channel handle from channel c's slices of the views: every
// kernel here calls the device function the shared operator's kernel calls (mg_coarsen_weighted_cell) or keeps its
// statements in their order (weighted_coef_cell, weighted_coef_fixed_cell: k_weighted_coef[_fixed]'s; k_pco_rhs:
// k_weighted_rhs's), with the channel on grid z.
//
// Storage.  The handle keeps `channels` sets of the four level-0 planes, 4 x ch_stride doubles apart (d, we, ws, lambda of
// a channel one after the other), and, while any channel has a fixed pixel, `channels` sets of ce, cs, lambda',
// 3 x ch_stride apart.  A channel without fixed pixels beside one that has some carries ce = cs = 0 and lambda' = lambda:
// w + 0.0 is w for every valid weight but -0.0, whose products are zeros that a sum started at +0.0 absorbs, so its
// right-hand side and hierarchy have the bits of a handle without the three extra planes.
//
// The kernels of this file are compiled in ccp_grid_pco.hip alone; ccp_grid.hip and ccp_grid_mg.hip include only
// ccp_grid_pco_api.hpp (PcoView and the launchers, no kernels), so their own device code does not change with this file.
#pragma once

#include "ccp_grid_mg.hpp"
#include "ccp_grid_mgb.hpp"
#include "ccp_grid_pco_api.hpp"
#include "ccp_grid_weighted.hpp"

namespace ccp {

// The planes' values at pixel (x,y) from the weight accessors wx, wy, lam (called as a(y, x)) and, in the second form, the
// mask of fixed pixels (fixed(y, x, 0) != 0 is fixed): the arithmetic at the top of ccp_grid_weighted.hpp, statement for
// statement that of k_weighted_coef / k_weighted_coef_fixed.  (Those two keep their own copy: routing them through these
// functions changes their register allocation, and the device code of ccp_grid.hip is kept byte-identical.)  ok: every
// weight the pixel owns is valid.
struct CoefCell {
    double d, we, ws, lam;
    bool ok;
};

template <typename WX, typename WY, typename WL>
__device__ __forceinline__ CoefCell weighted_coef_cell(const WX &wx, const WY &wy, const WL &lam, int x, int y, int W, int H)
{
    const double l = lam(y, x);
    const double e = x + 1 < W ? wx(y, x) : 0.0;
    const double s = y + 1 < H ? wy(y, x) : 0.0;
    double dd = l;
    if (y >= 1) dd += wy(y - 1, x);
    if (x >= 1) dd += wx(y, x - 1);
    if (x + 1 < W) dd += e;
    if (y + 1 < H) dd += s;
    return CoefCell{dd, e, s, l, weight_ok(l) && weight_ok(e) && weight_ok(s)};
}

struct CoefCellFixed {
    double d, we, ws, lam, ce, cs, lam_mg;
    bool ok;
    unsigned n_fixed, n_dead, n_edges;                                     // this pixel's share of the three counts
};

template <typename WX, typename WY, typename WL, typename M>
__device__ __forceinline__ CoefCellFixed weighted_coef_fixed_cell(const WX &wx, const WY &wy, const WL &lam, const M &fixed, int x, int y, int W,
                                                                  int H)
{
    const double l = lam(y, x);
    const double e = x + 1 < W ? wx(y, x) : 0.0;
    const double s = y + 1 < H ? wy(y, x) : 0.0;
    const bool fp = fixed(y, x, 0) != 0;
    const bool fN = y >= 1 && fixed(y - 1, x, 0) != 0, fW = x >= 1 && fixed(y, x - 1, 0) != 0;
    const bool fE = x + 1 < W && fixed(y, x + 1, 0) != 0, fS = y + 1 < H && fixed(y + 1, x, 0) != 0;
    const double wN = y >= 1 ? wy(y - 1, x) : 0.0, wW = x >= 1 ? wx(y, x - 1) : 0.0;
    double dd = l;
    if (y >= 1) dd += wN;
    if (x >= 1) dd += wW;
    if (x + 1 < W) dd += e;
    if (y + 1 < H) dd += s;
    double lp = l;
    if (fN) lp += wN;
    if (fW) lp += wW;
    if (fE) lp += e;
    if (fS) lp += s;
    const bool be = x + 1 < W && fp != fE, bs = y + 1 < H && fp != fS;   // edges with exactly one fixed end
    CoefCellFixed c;
    c.d = fp ? 0.0 : dd;
    c.we = fp || fE ? 0.0 : e;
    c.ws = fp || fS ? 0.0 : s;
    c.lam = fp ? -1.0 : l;
    c.ce = be ? e : 0.0;
    c.cs = bs ? s : 0.0;
    c.lam_mg = fp ? 0.0 : lp;
    c.ok = weight_ok(l) && weight_ok(e) && weight_ok(s);
    c.n_fixed = fp;
    c.n_dead = !fp && dd == 0.0;
    c.n_edges = (unsigned)be + (unsigned)bs;
    return c;
}

// channel c of a PcoView as the accessors weighted_coef_cell / weighted_coef_fixed_cell take: a(y, x) and m(y, x, 0)
struct PcoSlice {
    PcoView v;
    int c;
    __device__ __forceinline__ double operator()(int y, int x) const { return v(y, x, c); }
    __device__ __forceinline__ double operator()(int y, int x, int) const { return v(y, x, c); }
};

// d, we, ws, lambda of every pixel of every channel (k_weighted_coef, the channel on grid z): channel c's planes at
// op + c * op_stride, `plane` doubles apart.  One failure in any channel sets count[0].  grid = (ceil(W/kBlock), H, C).
static __global__ void __launch_bounds__(kBlock)
k_pco_coef(PcoView wx, PcoView wy, PcoView lam, int W, int H, long pitch, double *__restrict__ op, long plane, long op_stride,
           unsigned long long *__restrict__ count)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    if (x >= W) return;
    const CoefCell c = weighted_coef_cell(PcoSlice{wx, ch}, PcoSlice{wy, ch}, PcoSlice{lam, ch}, x, y, W, H);
    if (!c.ok) atomicOr(count, 1ull);
    double *__restrict__ o = op + (long)ch * op_stride;
    const long at = w_at(pitch, x, y);
    o[at] = c.d;
    o[plane + at] = c.we;
    o[2 * plane + at] = c.ws;
    o[3 * plane + at] = c.lam;
}

// k_pco_coef with a mask of fixed pixels per channel (k_weighted_coef_fixed, the channel on grid z): ce, cs, lambda' of
// channel c at cons + c * cons_stride.  count[0]: the verdict of all channels; count[1 + 3 c ..]: channel c's fixed
// pixels, free pixels with d = 0 and edges with exactly one fixed end -- per block in LDS, then one atomic per non-zero
// count.
static __global__ void __launch_bounds__(kBlock)
k_pco_coef_fixed(PcoView wx, PcoView wy, PcoView lam, PcoView fixed, int W, int H, long pitch, double *__restrict__ op, long plane,
                 long op_stride, double *__restrict__ cons, long cons_stride, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally[3];
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    unsigned n_fixed = 0, n_dead = 0, n_edges = 0;
    if (x < W) {
        const CoefCellFixed c =
            weighted_coef_fixed_cell(PcoSlice{wx, ch}, PcoSlice{wy, ch}, PcoSlice{lam, ch}, PcoSlice{fixed, ch}, x, y, W, H);
        if (!c.ok) atomicOr(count, 1ull);
        double *__restrict__ o = op + (long)ch * op_stride, *__restrict__ k = cons + (long)ch * cons_stride;
        const long at = w_at(pitch, x, y);
        o[at] = c.d;
        o[plane + at] = c.we;
        o[2 * plane + at] = c.ws;
        o[3 * plane + at] = c.lam;
        k[at] = c.ce;
        k[plane + at] = c.cs;
        k[2 * plane + at] = c.lam_mg;
        n_fixed = c.n_fixed;
        n_dead = c.n_dead;
        n_edges = c.n_edges;
    }
    if (n_fixed) atomicAdd(&tally[0], n_fixed);
    if (n_dead) atomicAdd(&tally[1], n_dead);
    if (n_edges) atomicAdd(&tally[2], n_edges);
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(count + 1 + 3 * ch + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// b of every channel from its OWN planes (k_weighted_rhs's order of operations, the channel on grid z instead of a loop
// over one set of weights): op, cons as above; gx, gy (f32), f, v (u8, f32 or f64) are H x W x C, has & 1: gx, & 2: gy,
// & 4: f, & 8: v, a missing one reads 0.  INIT: x := f on live pixels, 0 on dead ones.  FIXED: some channel has fixed
// pixels (cons is there).  grid = (ceil(W/kBlock), H, C).
template <bool INIT, bool FIXED>
__global__ void __launch_bounds__(kBlock)
k_pco_rhs(double *__restrict__ b, double *__restrict__ xo, Geom g, const double *__restrict__ op, long plane, long op_stride,
          const double *__restrict__ cons, long cons_stride, PcoView gx, PcoView gy, PcoView f, PcoView v, int has)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, c = blockIdx.z;
    if (x >= g.W) return;
    const double *__restrict__ d = op + (long)c * op_stride, *__restrict__ we = d + plane, *__restrict__ ws = d + 2 * plane,
                 *__restrict__ lam = d + 3 * plane;
    b += (long)c * g.ch_stride;
    xo += (long)c * g.ch_stride;
    const long at = w_at(g.pitch, x, y);
    double wN = y >= 1 ? ws[w_at(g.pitch, x, y - 1)] : 0.0, wW = x >= 1 ? we[w_at(g.pitch, x - 1, y)] : 0.0;
    double wE = we[at], wS = ws[at];
    const double l = lam[at];
    const bool live = d[at] != 0.0;
    const bool hx = has & 1, hy = has & 2, hf = has & 4, hv = has & 8;
    bool fN = false, fW = false, fE = false, fS = false;
    if (FIXED) {
        const double *__restrict__ ce = cons + (long)c * cons_stride, *__restrict__ cs = ce + plane;
        if (l < 0.0) {                                                      // a fixed pixel
            b[at] = 0.0;
            xo[at] = hv ? v(y, x, c) : 0.0;
            return;
        }
        if (y >= 1) {
            const long n = w_at(g.pitch, x, y - 1);
            wN += cs[n];
            fN = lam[n] < 0.0;
        }
        if (x >= 1) {
            const long w = w_at(g.pitch, x - 1, y);
            wW += ce[w];
            fW = lam[w] < 0.0;
        }
        wE += ce[at];
        wS += cs[at];
        fE = x + 1 < g.W && lam[w_at(g.pitch, x + 1, y)] < 0.0;
        fS = y + 1 < g.H && lam[w_at(g.pitch, x, y + 1)] < 0.0;
    }
    const double fv = hf ? f(y, x, c) : 0.0;
    double t = 0.0;
    if (y >= 1) t += wN * (hy ? gy(y - 1, x, c) : 0.0);
    if (x >= 1) t += wW * (hx ? gx(y, x - 1, c) : 0.0);
    if (x + 1 < g.W) t += -(wE * (hx ? gx(y, x, c) : 0.0));
    if (y + 1 < g.H) t += -(wS * (hy ? gy(y, x, c) : 0.0));
    t += l * fv;
    if (FIXED) {
        if (fN) t += wN * (hv ? v(y - 1, x, c) : 0.0);
        if (fW) t += wW * (hv ? v(y, x - 1, c) : 0.0);
        if (fE) t += wE * (hv ? v(y, x + 1, c) : 0.0);
        if (fS) t += wS * (hv ? v(y + 1, x, c) : 0.0);
    }
    b[at] = t;
    if (INIT) xo[at] = live ? fv : 0.0;
}

// Coarse cell (X,Y) of level k+1 of every channel from the channel's level k (k_mg_coarsen_weighted's cell, the channel
// on grid z): the fine level's d, we, ws are lv's pointers + ch * fs, its lambda lam + ch * ls; the coarse planes
// d, we, ws, lam_c + ch * cstride.  grid = (ceil(Wc/kBlock), Hc, C).
static __global__ void __launch_bounds__(kBlock)
k_pco_coarsen(MgLevel lv, long fs, const double *__restrict__ lam, long ls, MgLevel cv, double *__restrict__ d, double *__restrict__ we,
              double *__restrict__ ws, double *__restrict__ lam_c, long cstride, double edge)
{
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = blockIdx.y;
    if (X >= cv.W) return;
    const long ch = blockIdx.z;
    lv.d += ch * fs;
    lv.we += ch * fs;
    lv.ws += ch * fs;
    const long co = ch * cstride;
    mg_coarsen_weighted_cell(lv, lam + ch * ls, cv, X, Y, d + co, we + co, ws + co, lam_c + co, edge);
}

// ---- the batched mode (CCP_MG_CHANNELS_BATCHED) on one operator per channel ----------------------------------------------
// ccp_grid_mgb.hpp's kernels fetch the operator once per launch and loop over the channels inside a workgroup, because
// all channels share it.  Here no channel shares a coefficient with another, so the loop has nothing to share: the
// channel lies on grid z (a 256 x 256 level 0 has 32 tiles for 256 CUs; grid z multiplies that by C), and a block whose
// channel has stopped (st[ch].active == 0) returns before it loads anything.  Channel ch gets the bits of the sequential
// kernels: the per-cell functions are theirs (mg_nb_sum, mg_stored_update, mg_residual, mg_row0, mg_tail_body,
// block_sum), and every partial sum is grouped as k_mg_apply groups it (the same grid within a channel).  The vector
// and scalar passes do not touch the operator: k_mgb_init, _dot, _update, ... serve as they are.
//
// A level's per-channel coefficients: lv holds channel 0's d, we, ws; channel ch's are `os` doubles further.

__device__ __forceinline__ MgLevel pco_level(MgLevel lv, long os, int ch)
{
    lv.d += ch * os;
    lv.we += ch * os;
    lv.ws += ch * os;
    return lv;
}

// k_mg_tile<kMgCoarse, POST> for channel blockIdx.z: the region's d, we, ws are staged in LDS beside b and z (five fp64
// planes, mgb_tile_lds(kMgCoarse, nu), k_mgb_tile's layout and its 1,024 threads: which thread updates a cell does not
// change the cell's arithmetic), so no coefficient is read from global memory inside a half-sweep.  fs: the channel
// stride of b, z_in, z_out; es: of ec.  grid = (k_mg_tile's x, its y, C).
template <bool POST>
__global__ void __launch_bounds__(mgb_tile_threads(kMgCoarse))
k_pco_tile(MgLevel lv, long os, const double *__restrict__ b, const double *__restrict__ z_in, double *__restrict__ z_out, long fs, MgLevel cv,
           const double *__restrict__ ec, long es, double cs, int nu, const CgState *__restrict__ st)
{
    extern __shared__ double pco_lds[];
    constexpr int NT = mgb_tile_threads(kMgCoarse);
    const int ch = blockIdx.z;
    if (st && !st[ch].active) return;                                // (uniform) before any load
    const int h = 2 * nu, RW = kMgTileW + 2 * h, RH = kMgTileH + 2 * h, n = RW * RH;
    double *sb = pco_lds, *sz = pco_lds + n, *sd = pco_lds + 2 * n, *swe = pco_lds + 3 * n, *sws = pco_lds + 4 * n;
    const double *__restrict__ gd = lv.d + ch * os, *__restrict__ gwe = lv.we + ch * os, *__restrict__ gws = lv.ws + ch * os;
    const double *__restrict__ bc = b + ch * fs;
    const int x0 = blockIdx.x * kMgTileW - h, y0 = lv.lo + blockIdx.y * kMgTileH - h;
    for (int i = threadIdx.x; i < n; i += NT) {                      // outside the level: dead, every weight 0, b = z = 0
        const int x = x0 + i % RW, y = y0 + i / RW;
        double dv = 0.0, ev = 0.0, sv = 0.0, bv = 0.0, zv = 0.0;
        if (x >= 0 && x < lv.W && y >= 0 && y < lv.H) {
            const long at = mg_at(lv.pitch, x, y);
            dv = gd[at];
            ev = gwe[at];
            sv = gws[at];
            bv = bc[at];
            if (POST) {
                zv = z_in[ch * fs + at];
                if (dv != 0.0) zv = zv + cs * ec[ch * es + mg_at(cv.pitch, x >> 1, ((lv.y0 + y) >> 1) - cv.y0)];   // (cs * e_c is exact)
            }
        }
        sd[i] = dv;
        swe[i] = ev;
        sws[i] = sv;
        sb[i] = bv;
        sz[i] = zv;
    }
    __syncthreads();
    const int hw = RW / 2;
    auto half_sweep = [&](int c) {
        for (int k = threadIdx.x; k < hw * RH; k += NT) {
            const int r = k / hw, y = y0 + r;
            const int col = 2 * (k % hw) + ((c + y) & 1), x = x0 + col;
            if (x < 0 || x >= lv.W || y < 0 || y >= lv.H) continue;
            const int i = r * RW + col;
            const double xu = r > 0 ? sz[i - RW] : 0.0, xd = r + 1 < RH ? sz[i + RW] : 0.0;
            const double xl = col > 0 ? sz[i - 1] : 0.0, xr = col + 1 < RW ? sz[i + 1] : 0.0;
            const double d = sd[i];
            double out = 0.0;
            if (d != 0.0) {
                const double s = mg_nb_sum(r > 0 ? sws[i - RW] : 0.0, xu, col > 0 ? swe[i - 1] : 0.0, xl, swe[i], xr, sws[i], xd);
                out = mg_stored_update(sb[i], s, d);
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
}

// k_mg_restrict<kMgCoarse> for channel blockIdx.z (whole levels: Y0 = 0).  fs: the channel stride of b and z, es: of bc.
// grid = (ceil(Wc/kBlock), Hc, C).
static __global__ void __launch_bounds__(kBlock)
k_pco_restrict(MgLevel lv, long os, const double *__restrict__ b, const double *__restrict__ z, long fs, MgLevel cv, double *__restrict__ bc,
               long es, const CgState *__restrict__ st)
{
    const int ch = blockIdx.z;
    if (st && !st[ch].active) return;
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = blockIdx.y;
    if (X >= cv.W) return;
    const MgLevel l = pco_level(lv, os, ch);
    const double *__restrict__ bb = b + ch * fs, *__restrict__ zz = z + ch * fs;
    const int x = 2 * X, y = 2 * (cv.y0 + Y) - lv.y0;
    const double r00 = mg_residual<kMgCoarse>(l, bb, zz, x, y), r10 = mg_residual<kMgCoarse>(l, bb, zz, x + 1, y);
    const double r01 = mg_residual<kMgCoarse>(l, bb, zz, x, y + 1), r11 = mg_residual<kMgCoarse>(l, bb, zz, x + 1, y + 1);
    bc[ch * es + mg_at(cv.pitch, X, Y)] = (r00 + r10) + (r01 + r11);
}

// k_mg_apply<kMgCoarse, DOT> for channel blockIdx.z >> 1, colour blockIdx.z & 1: out := A_ch in_ch (vs: the channel stride
// of in and out).  DOT: channel ch's partial sums in its slice, partial + ch * ps, at k_mg_apply's index.
// grid = (k_mg_apply's x, its y, 2 C).
template <bool DOT>
__global__ void __launch_bounds__(kBlock)
k_pco_apply(MgLevel lv, long os, const double *__restrict__ in, double *__restrict__ out, long vs, double *__restrict__ partial, long ps,
            const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    const int c = blockIdx.z & 1, ch = blockIdx.z >> 1;
    if (st && !st[ch].active) return;                                // (uniform)
    const MgLevel l = pco_level(lv, os, ch);
    const double *__restrict__ zi = in + ch * vs;
    double *__restrict__ zo = out + ch * vs;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    double dot = 0.0;
    for (int y = l.lo + blockIdx.y; y < l.hi; y += gridDim.y) {
        const int x = 2 * j + ((y + c) & 1);
        if (x < l.W) {
            const long at = mg_at(l.pitch, x, y);
            const double ax = mg_row0<kMgCoarse>(l, zi, x, y);
            zo[at] = ax;
            dot += zi[at] * ax;
        }
    }
    if (DOT) {
        const double t = block_sum(dot, scratch);
        if (threadIdx.x == 0) partial[ch * ps + ((long)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// The tail: mg_tail_body, one workgroup per channel on the channel's own descriptor tails[blockIdx.x] (device memory, made
// with the hierarchy: a descriptor patched inside the kernel would be a private array indexed at run time).  bs, zs: the
// channel strides of b_top, z_top.
static __global__ void __launch_bounds__(kBlock)
k_pco_tail(const MgTail *__restrict__ tails, const double *__restrict__ b_top, double *__restrict__ z_top, long bs, long zs, double cs, int nu,
           const CgState *__restrict__ st)
{
    const int ch = blockIdx.x;
    if (st && !st[ch].active) return;
    mg_tail_body(tails[ch], b_top + ch * bs, z_top + ch * zs, cs, nu);
}

}  // namespace ccp
