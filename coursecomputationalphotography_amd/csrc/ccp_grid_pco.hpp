// ccp_grid_pco.hpp — the batched mode (CCP_MG_CHANNELS_BATCHED) of a weighted grid handle with one operator PER CHANNEL
// (include/ccp_gs.h, ccp_grid_set_weights_per_channel_device), hand-written for gfx950: the operator-dependent passes of
// the batched PCG (tile, restrict, tail, product) with the channel on a grid axis.  (The formation, the right-hand side
// and the coarsening of such a handle are the weighted handle's operator kernels, ccp_grid_weighted.hpp: they serve one
// operator and one per channel alike.)
//
// ccp_grid_mgb.hpp's kernels fetch the operator once per launch and loop over the channels inside a workgroup, because
// all channels share it.  Here no channel shares a coefficient with another, so the loop has nothing to share: the
// channel lies on grid z (a 256 x 256 level 0 has 32 tiles for 256 CUs; grid z multiplies that by C), and a block whose
// channel has stopped (st[ch].active == 0) returns before it loads anything.  Channel ch gets the bits of the sequential
// kernels: the per-cell functions are theirs (mg_nb_sum, mg_stored_update, mg_residual, mg_row0, mg_tail_body,
// block_sum), and every partial sum is grouped as k_mg_apply groups it (the same grid within a channel).  The vector
// and scalar passes do not touch the operator: k_mgb_init, _dot, _update, ... serve as they are.
//
// The kernels of this file are compiled in ccp_grid_weighted.hip alone; ccp_grid_mg.hip includes only
// ccp_grid_weighted_api.hpp (the launchers, no kernels), so its own device code does not change with this file.
#pragma once

#include "ccp_grid_mg.hpp"
#include "ccp_grid_mgb.hpp"
#include "ccp_grid_weighted_api.hpp"

namespace ccp {

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
