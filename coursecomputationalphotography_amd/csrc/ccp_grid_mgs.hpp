// ccp_grid_mgs.hpp — the fp32 V-cycle of the multigrid-preconditioned conjugate gradient (CCP_MG_PRECISION_F32,
// include/ccp_gs.h), hand-written for gfx950.  The fp64 V-cycle, the hierarchy and the layout: ccp_grid_mg.hpp.
//
// What it computes.  The hierarchy is built in fp64 as ever; every level's d, we, ws are then narrowed to float (round
// to nearest: k_mgs_narrow, which also gives the verdict of the narrowing) and a pixel is live if its float d != 0.
// z := M^-1 r narrows r once on the way in, runs ccp_grid_mg.hpp's V-cycle with every value a float -- the same sweeps,
// operation order, restriction order, cs, tile / tail / 1x1 structure -- and widens the result on the way out.  The
// division is IEEE (correctly rounded, denormals kept) and nothing is contracted to an fma.
//
// Where the conversions happen: in the level-0 kernels' loads and stores, never in a pass of their own.  B is the type
// of a level's right-hand side in memory (double on level 0: the PCG's r; float below), Z the type the tile kernel
// stores (double for the level-0 post-smoothing pass, which writes the PCG's z; float otherwise: t, and every coarse
// vector).  A weighted handle's level 0 reads float copies of its stored planes (12 B per pixel instead of 24).
//
// The tile in LDS is colour-split, like the levels in memory: cell (r, col) of the region sits in plane (r + col) & 1 of
// row r at half-column col >> 1.  The lanes of a half-sweep then read and write consecutive floats (a raster tile would
// put them 8 B apart: two lanes per bank for ds_read_b32), and the tile's loads and stores walk consecutive addresses of
// both the LDS and the level's planes.  The results do not depend on it.
//
// Single blocks only: a level holds its whole rows [0, H) (ccp_grid_mg_set_precision refuses row blocks).
#pragma once

#include "ccp_grid_mg.hpp"

namespace ccp {

constexpr int kMgsTileW = 64, kMgsTileH = 32;                     // output tile of k_mgs_tile (halo 2 nu around it), as k_mg_tile's

__host__ __device__ constexpr int mgs_tile_lds(int nu)
{
    return 2 * (kMgsTileW + 4 * nu) * (kMgsTileH + 4 * nu) * (int)sizeof(float);   // b and z of the tile and its halo
}

struct MgsLevel {
    int W, H;
    long pitch;
    const float *d, *we, *ws;         // coarse levels and a weighted handle's level 0 (narrowed planes)
    const unsigned char *mask;        // level 0 of a Dirichlet-mask grid
    Geom g0;                          // level 0: the image
};

// dst := (float)src over n values; *bad |= 1 if a value does not narrow to a finite one, |= 2 if a non-zero value
// narrows to zero.  grid = (ceil(n / kBlock)).
static __global__ void __launch_bounds__(kBlock)
k_mgs_narrow(const double *__restrict__ src, float *__restrict__ dst, long n, unsigned *__restrict__ bad)
{
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double v = src[i];
    const float f = (float)v;
    dst[i] = f;
    unsigned flag = 0;
    if (!(f >= -FLT_MAX && f <= FLT_MAX)) flag |= 1u;
    if (v != 0.0 && f == 0.0f) flag |= 2u;
    if (flag) atomicOr(bad, flag);
}

__device__ __forceinline__ float mgs_ld(const float *__restrict__ v, const MgsLevel &lv, int x, int y)
{
    return (x >= 0 && x < lv.W && y >= 0 && y < lv.H) ? v[mg_at(lv.pitch, x, y)] : 0.0f;
}

template <int KIND>
__device__ __forceinline__ bool mgs_live(const MgsLevel &lv, int x, int y)
{
    if (KIND == kMgSolve) return classify(lv.g0, x, y, y).diag != 0;
    if (KIND == kMgMasked) return lv.mask[mg_at(lv.pitch, x, y)] != 0;
    return lv.d[mg_at(lv.pitch, x, y)] != 0.0f;
}

// mg_update in float: one Gauss-Seidel update of (x,y) from b and the four neighbours' values (0 outside the level)
template <int KIND>
__device__ __forceinline__ float mgs_update(const MgsLevel &lv, float bv, float xu, float xl, float xr, float xd, int x, int y)
{
    const long at = mg_at(lv.pitch, x, y);
    if (KIND == kMgSolve) {                                          // gs_update
        const Stencil s = classify(lv.g0, x, y, y);
        if (s.diag == 0) return 0.0f;
        float sigma = 0.0f;
        if (s.up) sigma += -1.0f * xu;
        if (s.left) sigma += -1.0f * xl;
        if (s.right) sigma += -1.0f * xr;
        if (s.down) sigma += -1.0f * xd;
        return (bv - sigma) / (float)s.diag;
    } else if (KIND == kMgMasked) {
        return lv.mask[at] ? (bv + (((xu + xl) + xr) + xd)) * 0.25f : 0.0f;
    } else {
        const float d = lv.d[at];
        if (d == 0.0f) return 0.0f;
        float s = 0.0f;
        s += mgs_ld(lv.ws, lv, x, y - 1) * xu;
        s += mgs_ld(lv.we, lv, x - 1, y) * xl;
        s += lv.we[at] * xr;
        s += lv.ws[at] * xd;
        return (bv + s) / d;
    }
}

// mg_residual in float: b - A z at (x,y), b narrowed on load; 0 outside the level and on dead pixels
template <int KIND, typename B>
__device__ __forceinline__ float mgs_residual(const MgsLevel &lv, const B *__restrict__ b, const float *__restrict__ z, int x, int y)
{
    if (x >= lv.W || y >= lv.H) return 0.0f;
    const long at = mg_at(lv.pitch, x, y);
    const float xi = z[at];
    const float xu = mgs_ld(z, lv, x, y - 1), xl = mgs_ld(z, lv, x - 1, y), xr = mgs_ld(z, lv, x + 1, y), xd = mgs_ld(z, lv, x, y + 1);
    if (KIND == kMgSolve) {                                          // apply_row
        const Stencil s = classify(lv.g0, x, y, y);
        if (s.diag == 0) return 0.0f;
        float sum = 0.0f;
        if (s.up) sum += -1.0f * xu;
        if (s.left) sum += -1.0f * xl;
        sum += (float)s.diag * xi;
        if (s.right) sum += -1.0f * xr;
        if (s.down) sum += -1.0f * xd;
        return (float)b[at] - sum;
    } else if (KIND == kMgMasked) {
        if (!lv.mask[at]) return 0.0f;
        float ax = 0.0f;
        ax += -1.0f * xu;
        ax += -1.0f * xl;
        ax += 4.0f * xi;
        ax += -1.0f * xr;
        ax += -1.0f * xd;
        return (float)b[at] - ax;
    } else {
        const float d = lv.d[at];
        if (d == 0.0f) return 0.0f;
        float s = 0.0f;
        s += mgs_ld(lv.ws, lv, x, y - 1) * xu;
        s += mgs_ld(lv.we, lv, x - 1, y) * xl;
        s += lv.we[at] * xr;
        s += lv.ws[at] * xd;
        return (float)b[at] - (d * xi - s);
    }
}

// k_mg_restrict in float: the residual of the four children of coarse cell (X,Y), added up.  grid = (ceil(Wc/kBlock), Hc).
template <int KIND, typename B>
__global__ void __launch_bounds__(kBlock)
k_mgs_restrict(MgsLevel lv, const B *__restrict__ b, const float *__restrict__ z, MgsLevel cv, float *__restrict__ bc,
               const CgState *__restrict__ st)
{
    if (st && !st->active) return;
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = blockIdx.y;
    if (X >= cv.W) return;
    const int x = 2 * X, y = 2 * Y;
    const float r00 = mgs_residual<KIND>(lv, b, z, x, y), r10 = mgs_residual<KIND>(lv, b, z, x + 1, y);
    const float r01 = mgs_residual<KIND>(lv, b, z, x, y + 1), r11 = mgs_residual<KIND>(lv, b, z, x + 1, y + 1);
    bc[mg_at(cv.pitch, X, Y)] = (r00 + r10) + (r01 + r11);
}

// k_mg_tile in float (its comment explains the pass): all nu pre-smoothing sweeps from z = 0 (POST = false), or the
// prolongation z += cs * e_c on live pixels and all nu post-smoothing sweeps (POST = true), on a kMgsTileW x kMgsTileH
// tile with a halo of 2 nu cells, in LDS.  b is narrowed on load (B = double on level 0) and z widened on store (Z =
// double for the pass that writes the PCG's z).  z_in and z_out must be different buffers.  Bytes per cell of the tile
// below level 0: pre-smoothing b 4 x halo factor + z 4; post-smoothing (b, z 8 + e_c 1) x halo factor + z 4.
// grid = (ceil(W / kMgsTileW), ceil(H / kMgsTileH)); dynamic LDS mgs_tile_lds(nu) bytes.
template <int KIND, bool POST, typename B, typename Z>
__global__ void __launch_bounds__(kBlock)
k_mgs_tile(MgsLevel lv, const B *__restrict__ b, const float *__restrict__ z_in, Z *__restrict__ z_out, MgsLevel cv,
           const float *__restrict__ ec, float cs, int nu, const CgState *__restrict__ st)
{
    extern __shared__ float mgs_lds[];
    if (st && !st->active) return;                                   // (uniform)
    const int h = 2 * nu, RW = kMgsTileW + 2 * h, RH = kMgsTileH + 2 * h, hw = RW / 2, n = RW * RH;
    float *sb = mgs_lds, *sz = mgs_lds + n;
    // x0, y0 even: plane (r + col) & 1 of the region is the level's colour plane (x + y) & 1
    const int x0 = blockIdx.x * kMgsTileW - h, y0 = blockIdx.y * kMgsTileH - h;
    for (int i = threadIdx.x; i < n; i += kBlock) {                  // i = (r * 2 + plane) * hw + half-column
        const int rp = i / hw, r = rp >> 1, col = 2 * (i - rp * hw) + ((rp + r) & 1);
        const int x = x0 + col, y = y0 + r;
        float bv = 0.0f, zv = 0.0f;                                  // outside the level: 0, never updated
        if (x >= 0 && x < lv.W && y >= 0 && y < lv.H) {
            const long at = mg_at(lv.pitch, x, y);
            bv = (float)b[at];
            if (POST) {
                zv = z_in[at];
                if (mgs_live<KIND>(lv, x, y)) zv = zv + cs * ec[mg_at(cv.pitch, x >> 1, y >> 1)];   // (cs * e_c is exact)
            }
        }
        sb[i] = bv;
        sz[i] = zv;
    }
    __syncthreads();
    auto half_sweep = [&](int c) {
        for (int k = threadIdx.x; k < hw * RH; k += kBlock) {
            const int r = k / hw, j = k - r * hw, y = y0 + r;
            const int q = (c + r) & 1, col = 2 * j + q, x = x0 + col;
            if (x < 0 || x >= lv.W || y < 0 || y >= lv.H) continue;
            const int i = (2 * r + c) * hw + j;                      // the cell; its neighbours are in plane 1 - c
            const int o = (2 * r + 1 - c) * hw + j;                  // the other plane of this row at j: column col - 1 + 2 q
            const float xu = r > 0 ? sz[o - 2 * hw] : 0.0f, xd = r + 1 < RH ? sz[o + 2 * hw] : 0.0f;
            const float xl = col > 0 ? sz[o - 1 + q] : 0.0f, xr = col + 1 < RW ? sz[o + q] : 0.0f;
            sz[i] = mgs_update<KIND>(lv, sb[i], xu, xl, xr, xd, x, y);
        }
        __syncthreads();
    };
    for (int s = 0; s < nu; ++s) {
        half_sweep(POST ? 1 : 0);
        half_sweep(POST ? 0 : 1);
    }
    constexpr int thw = kMgsTileW / 2;
    for (int k = threadIdx.x; k < kMgsTileW * kMgsTileH; k += kBlock) {   // k = (row * 2 + plane) * thw + half-column
        const int rp = k / thw, r = h + (rp >> 1), p = (rp + (rp >> 1)) & 1, col = h + 2 * (k - rp * thw) + p;
        const int x = x0 + col, y = y0 + r;
        if (x < lv.W && y < lv.H) z_out[mg_at(lv.pitch, x, y)] = (Z)sz[(2 * r + ((r + col) & 1)) * hw + (col >> 1)];
    }
}

// ---- the tail: k_mg_tail in float (every level from the tail's first down to 1x1 in one workgroup, resident in LDS) ----
struct MgsTail {
    int levels;
    int W[kMgTailLevels], H[kMgTailLevels], off[kMgTailLevels];
    long pitch[kMgTailLevels];
    const float *d[kMgTailLevels], *we[kMgTailLevels], *ws[kMgTailLevels];
};

static __global__ void __launch_bounds__(kBlock)
k_mgs_tail(MgsTail t, const float *__restrict__ b_top, float *__restrict__ z_top, float cs, int nu, const CgState *__restrict__ st)
{
    if (st && !st->active) return;
    __shared__ float sd[kMgTailCells], swe[kMgTailCells], sws[kMgTailCells], sb[kMgTailCells], sz[kMgTailCells];
    for (int k = 0; k < t.levels; ++k) {
        const int W = t.W[k], n = t.W[k] * t.H[k];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const long at = mg_at(t.pitch[k], i % W, i / W);
            sd[t.off[k] + i] = t.d[k][at];
            swe[t.off[k] + i] = t.we[k][at];
            sws[t.off[k] + i] = t.ws[k][at];
            if (k == 0) sb[i] = b_top[at];
        }
    }
    __syncthreads();
    auto sum_nb = [&](int k, int X, int Y, float &xi) -> float {
        const int W = t.W[k], H = t.H[k], o = t.off[k], i = o + Y * W + X;
        xi = sz[i];
        float s = 0.0f;
        s += (Y > 0 ? sws[i - W] : 0.0f) * (Y > 0 ? sz[i - W] : 0.0f);
        s += (X > 0 ? swe[i - 1] : 0.0f) * (X > 0 ? sz[i - 1] : 0.0f);
        s += swe[i] * (X + 1 < W ? sz[i + 1] : 0.0f);
        s += sws[i] * (Y + 1 < H ? sz[i + W] : 0.0f);
        return s;
    };
    auto sweep = [&](int k, int c, bool first) {
        const int W = t.W[k], n = t.W[k] * t.H[k], o = t.off[k];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int X = i % W, Y = i / W;
            if (((X + Y) & 1) != c) continue;
            const float d = sd[o + i];
            float v = 0.0f;
            if (d != 0.0f) {
                float xi;
                const float s = first ? 0.0f : sum_nb(k, X, Y, xi);
                v = (sb[o + i] + s) / d;
            }
            sz[o + i] = v;
        }
        __syncthreads();
    };
    auto residual = [&](int k, int X, int Y) -> float {
        if (X >= t.W[k] || Y >= t.H[k]) return 0.0f;
        const int i = t.off[k] + Y * t.W[k] + X;
        const float d = sd[i];
        if (d == 0.0f) return 0.0f;
        float xi;
        const float s = sum_nb(k, X, Y, xi);
        return sb[i] - (d * xi - s);
    };
    const int last = t.levels - 1;
    for (int k = 0; k < last; ++k) {
        for (int s = 0; s < nu; ++s) {
            sweep(k, 0, s == 0);
            sweep(k, 1, false);
        }
        const int Wc = t.W[k + 1], nc = t.W[k + 1] * t.H[k + 1], oc = t.off[k + 1];
        for (int i = threadIdx.x; i < nc; i += kBlock) {
            const int X = i % Wc, Y = i / Wc;
            const float r00 = residual(k, 2 * X, 2 * Y), r10 = residual(k, 2 * X + 1, 2 * Y);
            const float r01 = residual(k, 2 * X, 2 * Y + 1), r11 = residual(k, 2 * X + 1, 2 * Y + 1);
            sb[oc + i] = (r00 + r10) + (r01 + r11);
        }
        __syncthreads();
    }
    {
        const int n = t.W[last] * t.H[last], o = t.off[last];
        for (int i = threadIdx.x; i < n; i += kBlock) sz[o + i] = sd[o + i] != 0.0f ? sb[o + i] / sd[o + i] : 0.0f;
        __syncthreads();
    }
    for (int k = last - 1; k >= 0; --k) {
        const int W = t.W[k], n = t.W[k] * t.H[k], o = t.off[k], Wc = t.W[k + 1], oc = t.off[k + 1];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int X = i % W, Y = i / W;
            if (sd[o + i] != 0.0f) sz[o + i] = sz[o + i] + cs * sz[oc + (Y >> 1) * Wc + (X >> 1)];
        }
        __syncthreads();
        for (int s = 0; s < nu; ++s) {
            sweep(k, 1, false);
            sweep(k, 0, false);
        }
    }
    const int W = t.W[0], n = t.W[0] * t.H[0];
    for (int i = threadIdx.x; i < n; i += kBlock) z_top[mg_at(t.pitch[0], i % W, i / W)] = sz[i];
}

}  // namespace ccp
