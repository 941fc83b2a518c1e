// ccp_grid_mgs.hpp — the fp32 V-cycle of the multigrid-preconditioned conjugate gradient (CCP_MG_PRECISION_F32,
// include/ccp_gs.h), hand-written for gfx950.  The fp64 V-cycle, the hierarchy and the layout: ccp_grid_mg.hpp.
//
// What it computes.  The hierarchy is built in fp64 as ever; every level's d, we, ws are then narrowed to float (round
// to nearest: k_mgs_narrow, which also gives the verdict of the narrowing) and a pixel is live if its float d != 0.
// z := M^-1 r narrows r once on the way in, runs ccp_grid_mg.hpp's V-cycle with every value a float -- the same sweeps,
// operation order, restriction order, cs, tile / tail / 1x1 structure -- and widens the result on the way out.  The
// per-cell formulas and the tail's cycle are ccp_grid_mg.hpp's own templates (mg_nb_sum .., mg_tail_body) and
// ccp_grid_stencil.hpp's gs_update / apply_row, instantiated for float; the level struct, the loads and the tile kernel
// (colour-split LDS) are this file's.  The division is IEEE (correctly rounded, denormals kept) and nothing is
// contracted to an fma.
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

#include <cfloat>

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

// mg_update on floats: one Gauss-Seidel update of (x,y) from b and the four neighbours' values (0 outside the level), by
// the formulas mg_update uses
template <int KIND>
__device__ __forceinline__ float mgs_update(const MgsLevel &lv, float bv, float xu, float xl, float xr, float xd, int x, int y)
{
    const long at = mg_at(lv.pitch, x, y);
    if (KIND == kMgSolve) {
        float out = 0.0f;
        return gs_update(classify(lv.g0, x, y, y), bv, xu, xl, xr, xd, out) ? out : 0.0f;
    } else if (KIND == kMgMasked) {
        return lv.mask[at] ? mg_masked_update(bv, xu, xl, xr, xd) : 0.0f;
    } else {
        const float d = lv.d[at];
        if (d == 0.0f) return 0.0f;
        const float s = mg_nb_sum(mgs_ld(lv.ws, lv, x, y - 1), xu, mgs_ld(lv.we, lv, x - 1, y), xl, lv.we[at], xr, lv.ws[at], xd);
        return mg_stored_update(bv, s, d);
    }
}

// mg_residual on floats: b - A z at (x,y), b narrowed on load; 0 outside the level and on dead pixels
template <int KIND, typename B>
__device__ __forceinline__ float mgs_residual(const MgsLevel &lv, const B *__restrict__ b, const float *__restrict__ z, int x, int y)
{
    if (x >= lv.W || y >= lv.H) return 0.0f;
    const long at = mg_at(lv.pitch, x, y);
    const float xi = z[at];
    const float xu = mgs_ld(z, lv, x, y - 1), xl = mgs_ld(z, lv, x - 1, y), xr = mgs_ld(z, lv, x + 1, y), xd = mgs_ld(z, lv, x, y + 1);
    if (KIND == kMgSolve) {
        // apply_row adds the diagonal under `if (s.diag != 0)`; after the early return that is every time: the same bits
        const Stencil s = classify(lv.g0, x, y, y);
        if (s.diag == 0) return 0.0f;
        return (float)b[at] - apply_row(s, xi, xu, xl, xr, xd);
    } else if (KIND == kMgMasked) {
        if (!lv.mask[at]) return 0.0f;
        return (float)b[at] - mg_masked_row(xi, xu, xl, xr, xd);
    } else {
        const float d = lv.d[at];
        if (d == 0.0f) return 0.0f;
        const float s = mg_nb_sum(mgs_ld(lv.ws, lv, x, y - 1), xu, mgs_ld(lv.we, lv, x - 1, y), xl, lv.we[at], xr, lv.ws[at], xd);
        return mg_stored_residual((float)b[at], d, xi, s);
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

// ---- the tail: mg_tail_body (ccp_grid_mg.hpp) on floats, every level from the tail's first down to 1x1 in one workgroup ----
using MgsTail = MgTailT<float>;

static __global__ void __launch_bounds__(kBlock)
k_mgs_tail(MgsTail t, const float *__restrict__ b_top, float *__restrict__ z_top, float cs, int nu, const CgState *__restrict__ st)
{
    if (st && !st->active) return;
    mg_tail_body(t, b_top, z_top, cs, nu);
}

}  // namespace ccp
