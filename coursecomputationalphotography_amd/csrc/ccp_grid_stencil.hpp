// ccp_grid_stencil.hpp — the grid layout (Geom, row_off), 16-byte lane vectors and the 5-point stencil of
// SolveChannel's matrix (classify, gs_update, apply_row): the device helpers of ccp_grid_kernels.hpp, which explains
// the layout and the arithmetic; and the layout and the row of a weighted handle's stored operator (w_at, weighted_row).
// No kernels here, so that more than one translation unit may include it.
#pragma once

#include "ccp_common.hpp"
#include "ccp_grid_geom.hpp"       // Geom

namespace ccp {

__device__ __forceinline__ long row_off(const Geom &g, int l, int c)
{
    return ((long)l * 2 + c) * g.pitch;
}

template <int CPT>
__device__ __forceinline__ void ld_vec(const double *__restrict__ p, double (&v)[CPT])
{
    static_assert(CPT % 2 == 0, "CPT must be even (16-byte lane accesses)");
#pragma unroll
    for (int k = 0; k < CPT; k += 2) {
        const double2 t = *reinterpret_cast<const double2 *>(p + k);
        v[k] = t.x;
        v[k + 1] = t.y;
    }
}

template <int CPT>
__device__ __forceinline__ void st_vec(double *__restrict__ p, const double (&v)[CPT])
{
#pragma unroll
    for (int k = 0; k < CPT; k += 2) {
        double2 t;
        t.x = v[k];
        t.y = v[k + 1];
        *reinterpret_cast<double2 *>(p + k) = t;
    }
}

template <int CPT>
__device__ __forceinline__ void zero_vec(double (&v)[CPT])
{
#pragma unroll
    for (int k = 0; k < CPT; ++k) v[k] = 0.0;
}

// Which neighbours pixel (x,y) has in the reference matrix and its diagonal:
// cell(x,y) <=> x < W-1 && y < H-1 (the forward-difference loop bounds, PhotoMontage.cpp:551-554).
struct Stencil {
    bool up, left, right, down;
    int diag;
};

__device__ __forceinline__ Stencil classify(const Geom &g, int x, int y, int l)
{
    Stencil s;
    const bool here = (x < g.W - 1) && (y < g.H - 1);
    const bool cf_up = (y >= 1) && (x < g.W - 1);
    s.left = (x >= 1) && (y < g.H - 1);
    s.right = here;
    s.diag = (int)cf_up + (int)s.left + 2 * (int)here + (int)((x | y) == 0);
    // a neighbour row outside the local block (beyond the ghosts) is treated as absent; such
    // rows are never inside the sweep range of a correctly driven handle.
    s.up = cf_up && (l >= 1);
    s.down = here && (l + 1 < g.local_rows);
    return s;
}

// (b - sigma) / a_ii with the reference's accumulation order.  Returns false when the row is
// skipped (a_ii == 0, sparse-matrix.h:361-363).  T is deduced from the values: double everywhere
// but in the fp32 V-cycle (ccp_grid_mgs.hpp), which runs the same statement on floats.
template <typename T>
__device__ __forceinline__ bool gs_update(const Stencil &s, T bv, T xu, T xl, T xr, T xd, T &out)
{
    if (s.diag == 0) return false;
    T sigma = T(0);
    if (s.up) sigma += T(-1) * xu;
    if (s.left) sigma += T(-1) * xl;
    if (s.right) sigma += T(-1) * xr;
    if (s.down) sigma += T(-1) * xd;
    out = (bv - sigma) / (T)s.diag;
    return true;
}

// A x for one pixel in applyToVector's order (sparse-matrix.h:382-393): up, left, diagonal,
// right, down; empty rows give 0.  T as gs_update's.
template <typename T>
__device__ __forceinline__ T apply_row(const Stencil &s, T xi, T xu, T xl, T xr, T xd)
{
    T sum = T(0);
    if (s.up) sum += T(-1) * xu;
    if (s.left) sum += T(-1) * xl;
    if (s.diag != 0) sum += (T)s.diag * xi;
    if (s.right) sum += T(-1) * xr;
    if (s.down) sum += T(-1) * xd;
    return sum;
}

// ---- the weighted handles' stored operator (ccp_grid_weighted.hpp explains the planes) ---------------------------------
// cell (x,y) of a plane in the colour-split layout of x, b and the operator's planes
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

// lane i <- lane i-1 (lane 0 gets 0) / lane i <- lane i+1 (lane 63 gets 0): the strip-edge lanes
// have no neighbour inside the wave; their pixels are halo (never stored) or image-edge pixels
// whose stencil has no such neighbour.
__device__ __forceinline__ double lane_prev(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true);   // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_next(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);   // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

}  // namespace ccp
