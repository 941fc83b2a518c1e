// ccp_grid_weighted.hpp — the weighted grid handles (include/ccp_gs.h, CCP_GRID_WEIGHTED), hand-written for gfx950:
// the operator's formation with its validation, the right-hand side of every channel, and b := A x / the residual.
//
// Operator.  A weighted handle stores its level-0 operator in four planes of the grid's colour-split layout (w_at,
// the layout of x and b and of the multigrid levels' mg_at): d, we, ws and lambda, pads zero.  we / ws are the weights
// of the edges to the east / south cell (0 where the edge is absent); the weights from the north and west are the
// neighbours' ws / we.  The multigrid V-cycle runs level 0 as a stored operator (kMgCoarse, ccp_grid_mg.hpp) on these
// planes, and its coarsening carries lambda (k_mg_coarsen_weighted).
//
// Arithmetic (the header's formulas): d = lambda; d += wN; d += wW; d += wE; d += wS (terms whose edge lies outside
// the canvas skipped); t = 0; t += wN gy(x,y-1); t += wW gx(x-1,y); t += -(wE gx); t += -(wS gy); t += lambda f;
// A z = 0; += -(wN zN); += -(wW zW); += d z; += -(wE zE); += -(wS zS), 0 on dead pixels (d == 0).
//
// Fixed pixels (ccp_grid_set_weights_constrained_*).  With a non-empty set F of fixed pixels a free pixel keeps the d
// above, its stored we / ws is the weight where both ends of the edge are free and 0 otherwise, and a fixed pixel is dead
// (d = we = ws = 0).  Three more planes exist then: ce / cs, the weight of the east / south edge where exactly ONE of
// its ends is fixed (so that we + ce and ws + cs are the original weights, exactly: one of the two is 0), and
// lambda' = lambda; += cN; += cW; += cE; += cS (terms of free neighbours skipped; 0 on fixed pixels), the plane the
// multigrid hierarchy carries.  The lambda plane keeps the caller's lambda for the right-hand side and marks the fixed
// pixels: -1 there (a valid lambda is >= 0).  b of a free pixel is the t above from the ORIGINAL weights, then
// t += cN v(x,y-1); += cW v(x-1,y); += cE v(x+1,y); += cS v(x,y+1) over the fixed neighbours (v: the prescribed
// values); a fixed pixel gets b = 0 and x := v.
#pragma once

#include "ccp_grid_stencil.hpp"

#include <cfloat>

namespace ccp {

__host__ __device__ __forceinline__ long w_at(long pitch, int x, int y)
{
    return ((long)y * 2 + ((x + y) & 1)) * pitch + (x >> 1);
}

// (A z)(x,y) of the stored operator on a W x H single-block level (the PCG's product on level 0 as well)
__device__ __forceinline__ double weighted_row(const double *__restrict__ d, const double *__restrict__ we, const double *__restrict__ ws,
                                               long pitch, int W, int H, const double *__restrict__ z, int x, int y)
{
    const long at = w_at(pitch, x, y);
    const double dd = d[at];
    if (dd == 0.0) return 0.0;
    double a = 0.0;
    if (y >= 1) {
        const long n = w_at(pitch, x, y - 1);
        a += -(ws[n] * z[n]);
    }
    if (x >= 1) {
        const long w = w_at(pitch, x - 1, y);
        a += -(we[w] * z[w]);
    }
    a += dd * z[at];
    if (x + 1 < W) a += -(we[at] * z[w_at(pitch, x + 1, y)]);
    if (y + 1 < H) a += -(ws[at] * z[w_at(pitch, x, y + 1)]);
    return a;
}

// One H x W weight array of ccp_grid_set_weights_*: f32 or f64 elements `sy`, `sx` apart (0: broadcast), or none
// (p == nullptr): the default value everywhere.
struct WeightView {
    const void *p;
    long sy, sx;
    int f64;
    double dflt;
    __device__ __forceinline__ double operator()(int y, int x) const
    {
        if (!p) return dflt;
        const long i = (long)y * sy + (long)x * sx;
        return f64 ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
    }
};

__device__ __forceinline__ bool weight_ok(double v) { return v >= 0.0 && v <= DBL_MAX; }   // finite and >= 0 (NaN fails)

// d, we, ws, lambda of every pixel (one plane each, the layout of one channel of x).  Every weight is checked by the
// pixel that owns it (wx(x,y) and wy(x,y) by (x,y), where they are read); one failure sets *bad.  grid = (ceil(W/kBlock), H).
static __global__ void __launch_bounds__(kBlock)
k_weighted_coef(WeightView wx, WeightView wy, WeightView lam, int W, int H, long pitch, double *__restrict__ d,
                double *__restrict__ we, double *__restrict__ ws, double *__restrict__ lam_out, unsigned *__restrict__ bad)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const double l = lam(y, x);
    const double e = x + 1 < W ? wx(y, x) : 0.0;
    const double s = y + 1 < H ? wy(y, x) : 0.0;
    if (!(weight_ok(l) && weight_ok(e) && weight_ok(s))) atomicOr(bad, 1u);
    double dd = l;
    if (y >= 1) dd += wy(y - 1, x);
    if (x >= 1) dd += wx(y, x - 1);
    if (x + 1 < W) dd += e;
    if (y + 1 < H) dd += s;
    const long at = w_at(pitch, x, y);
    d[at] = dd;
    we[at] = e;
    ws[at] = s;
    lam_out[at] = l;
}

// k_weighted_coef with a mask of fixed pixels (M: a View of u8, f32 or f64, != 0 is fixed): the planes described at the
// top, every weight checked as there (the fixed pixels' weights too).  count[0]: the verdict; count[1..3]: fixed pixels,
// free pixels with d = 0, edges with exactly one fixed end -- per block in LDS, then one atomic per non-zero count.
template <typename M>
__global__ void __launch_bounds__(kBlock)
k_weighted_coef_fixed(WeightView wx, WeightView wy, WeightView lam, M fixed, int W, int H, long pitch, double *__restrict__ d,
                      double *__restrict__ we, double *__restrict__ ws, double *__restrict__ lam_out, double *__restrict__ ce,
                      double *__restrict__ cs, double *__restrict__ lam_mg, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally[3];
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    unsigned n_fixed = 0, n_dead = 0, n_edges = 0;
    if (x < W) {
        const double l = lam(y, x);
        const double e = x + 1 < W ? wx(y, x) : 0.0;
        const double s = y + 1 < H ? wy(y, x) : 0.0;
        if (!(weight_ok(l) && weight_ok(e) && weight_ok(s))) atomicOr(count, 1ull);
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
        const long at = w_at(pitch, x, y);
        d[at] = fp ? 0.0 : dd;
        we[at] = fp || fE ? 0.0 : e;
        ws[at] = fp || fS ? 0.0 : s;
        lam_out[at] = fp ? -1.0 : l;
        ce[at] = be ? e : 0.0;
        cs[at] = bs ? s : 0.0;
        lam_mg[at] = fp ? 0.0 : lp;
        n_fixed = fp;
        n_dead = !fp && dd == 0.0;
        n_edges = (unsigned)be + (unsigned)bs;
    }
    if (n_fixed) atomicAdd(&tally[0], n_fixed);
    if (n_dead) atomicAdd(&tally[1], n_dead);
    if (n_edges) atomicAdd(&tally[2], n_edges);
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(count + 1 + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// pixels with d = 0 of an operator without fixed pixels (ccp_grid_constraint_info): one atomic per block that has any
static __global__ void __launch_bounds__(kBlock)
k_weighted_count_dead(const double *__restrict__ d, int W, int H, long pitch, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally;
    if (threadIdx.x == 0) tally = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x < W && d[w_at(pitch, x, y)] == 0.0) atomicAdd(&tally, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && tally) atomicAdd(count, (unsigned long long)tally);
}

// b of all C channels from the stored operator (op: d, we, ws, lambda planes `plane` doubles apart) and the guidance
// gx, gy / data f (accessors G, F: Views of the caller's arrays or of a host entry point's staging; has & 1: gx, has &
// 2: gy, has & 4: f, a missing one reads 0).  INIT: x := f on live pixels, 0 on dead ones.  grid = (ceil(W/kBlock), H).
// FIXED: the operator has fixed pixels (the planes ce, cs at `cons`, `plane` doubles apart; the lambda plane < 0 marks
// them): the guidance terms take the original weights we + ce, ws + cs, the prescribed values v (accessor V; has & 8,
// a missing one reads 0) of the fixed neighbours enter b, and a fixed pixel gets b = 0, x := v.
template <bool INIT, bool FIXED, typename G, typename F, typename V>
__global__ void __launch_bounds__(kBlock)
k_weighted_rhs(double *__restrict__ b, double *__restrict__ xo, Geom g, const double *__restrict__ op, long plane, G gx, G gy, F f,
               int has, int C, const double *__restrict__ cons, V v)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x >= g.W) return;
    const double *__restrict__ d = op, *__restrict__ we = op + plane, *__restrict__ ws = op + 2 * plane, *__restrict__ lam = op + 3 * plane;
    const long at = w_at(g.pitch, x, y);
    double wN = y >= 1 ? ws[w_at(g.pitch, x, y - 1)] : 0.0, wW = x >= 1 ? we[w_at(g.pitch, x - 1, y)] : 0.0;
    double wE = we[at], wS = ws[at];
    const double l = lam[at];
    const bool live = d[at] != 0.0;
    const bool hx = has & 1, hy = has & 2, hf = has & 4, hv = has & 8;
    bool fN = false, fW = false, fE = false, fS = false;
    if (FIXED) {
        const double *__restrict__ ce = cons, *__restrict__ cs = cons + plane;
        if (l < 0.0) {                                                      // a fixed pixel
            for (int c = 0; c < C; ++c) {
                b[(long)c * g.ch_stride + at] = 0.0;
                xo[(long)c * g.ch_stride + at] = hv ? (double)v(y, x, c) : 0.0;
            }
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
    for (int c = 0; c < C; ++c) {
        const double fv = hf ? (double)f(y, x, c) : 0.0;
        double t = 0.0;
        if (y >= 1) t += wN * (hy ? (double)gy(y - 1, x, c) : 0.0);
        if (x >= 1) t += wW * (hx ? (double)gx(y, x - 1, c) : 0.0);
        if (x + 1 < g.W) t += -(wE * (hx ? (double)gx(y, x, c) : 0.0));
        if (y + 1 < g.H) t += -(wS * (hy ? (double)gy(y, x, c) : 0.0));
        t += l * fv;
        if (FIXED) {
            if (fN) t += wN * (hv ? (double)v(y - 1, x, c) : 0.0);
            if (fW) t += wW * (hv ? (double)v(y, x - 1, c) : 0.0);
            if (fE) t += wE * (hv ? (double)v(y, x + 1, c) : 0.0);
            if (fS) t += wS * (hv ? (double)v(y + 1, x, c) : 0.0);
        }
        b[(long)c * g.ch_stride + at] = t;
        if (INIT) xo[(long)c * g.ch_stride + at] = live ? fv : 0.0;
    }
}

// MODE 0: b := A x; MODE 1: per (channel, colour) block partial sums of (b - A x)^2 and b^2 at
// partial[2 ((ch * 2 + c) * gridDim.x + blockIdx.x) + {0, 1}] (k_pair_reduce's layout, gridDim.x blocks per group).
// grid = (blocks, 1, 2 channels); a block strides over the cells of colour c.
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_weighted_apply(const double *__restrict__ x, double *__restrict__ b, Geom g, const double *__restrict__ op, long plane,
                 double *__restrict__ partial)
{
    __shared__ double scratch[kBlock / kWave];
    const int ch = blockIdx.z >> 1, c = blockIdx.z & 1;
    const double *__restrict__ d = op, *__restrict__ we = op + plane, *__restrict__ ws = op + 2 * plane;
    const double *__restrict__ xc = x + (long)ch * g.ch_stride;
    double *__restrict__ bc = b + (long)ch * g.ch_stride;
    const int hw = (g.W + 1) / 2;
    const long cells = (long)g.H * hw;
    double rr = 0.0, bb = 0.0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (long)gridDim.x * kBlock) {
        const int y = (int)(i / hw), xi = 2 * (int)(i - (long)y * hw) + ((y + c) & 1);
        if (xi >= g.W) continue;
        const double ax = weighted_row(d, we, ws, g.pitch, g.W, g.H, xc, xi, y);
        const long at = w_at(g.pitch, xi, y);
        if (MODE == 0) {
            bc[at] = ax;
        } else {
            const double bv = bc[at], r = bv - ax;
            rr += r * r;
            bb += bv * bv;
        }
    }
    if (MODE == 1) {
        const double t0 = block_sum(rr, scratch);
        const double t1 = block_sum(bb, scratch);
        if (threadIdx.x == 0) {
            const long k = 2 * ((long)blockIdx.z * gridDim.x + blockIdx.x);
            partial[k] = t0;
            partial[k + 1] = t1;
        }
    }
}

}  // namespace ccp
