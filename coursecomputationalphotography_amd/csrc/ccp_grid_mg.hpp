// ccp_grid_mg.hpp — geometric multigrid V-cycle as the preconditioner of conjugate gradient on the grid handles
// (ccp_grid_mg_conjugate_gradient, include/ccp_gs.h), hand-written for gfx950.
//
// Hierarchy.  Level 0 is the handle's own operator: SolveChannel's matrix (classify), the Dirichlet-mask Laplacian, or
// the stored operator of a weighted handle (kind kMgCoarse on the handle's d, we, ws planes: ccp_grid_weighted.hpp).
// Level k+1 is ceil(W_k/2) x ceil(H_k/2); coarse cell (X,Y) aggregates the live pixels (diagonal != 0) among
// (2X..2X+1, 2Y..2Y+1), down to 1x1.  A_{k+1} = P^T A_k P with P piecewise constant over the aggregates is again a
// 5-point operator, stored per cell as d (diagonal), we (weight to the east cell), ws (weight to the south cell);
// the weights are the positive couplings (A_ij = -w).  Every value is a small integer: exact in fp64.  A weighted
// hierarchy carries the data weight lambda on every level too and forms d without cancellation (k_weighted_coarsen):
// its weights are real numbers, and d - 2 x internal edges could round to a tiny or negative diagonal.
//
// Layout.  Every level uses the fine grid's colour-split layout: cell (X,Y) sits in colour plane (X+Y)&1 of row Y at
// half-column X>>1, pitch a multiple of 16 (mg_at).  Aggregate X of rows 2Y, 2Y+1 is half-column X of both planes of
// both rows.  Pads are zero and never written.
//
// V-cycle z = M^-1 r, every level from z = 0: nu red-black sweeps (red, black); residual restricted as
// rc = (r(2X,2Y) + r(2X+1,2Y)) + (r(2X,2Y+1) + r(2X+1,2Y+1)); recurse; z += 2.0 * e_c on live pixels; nu sweeps
// (black, red: M stays symmetric).  1x1: z = b/d (0 if dead).  Level 0 keeps the existing arithmetic bit for bit
// (gs_update / apply_row, the masked kernels' interior formula); coarse levels s = 0; s += wN xN; s += wW xW;
// s += wE xE; s += wS xS; x = (b + s) / d; r = b - (d x - s).  Dead pixels are written 0 by every sweep.
//
// The 2.0 is the hierarchy's correction scale, a uniform kernel argument `cs`: a weighted handle's rescaled hierarchy
// (CCP_MG_HIERARCHY_RESCALED: its coarsening halves the edge weights once per level and leaves lambda alone) passes 1.0,
// everything else 2.0.  cs * e_c is exact for both, so z + cs * e_c gives the same bits whether or not the compiler
// contracts it to an fma.
//
// The levels whose sides are both <= kMgTailSide (below level 0) run in ONE single-workgroup launch, k_mg_tail, with
// all of them resident in LDS (at most kMgTailCells cells x 5 doubles = 54.6 KB).  Every other level takes three
// launches: the nu pre-smoothing sweeps in one pass (k_mg_tile), residual + restriction (k_mg_restrict), prolongation
// + the nu post-smoothing sweeps in one pass (k_mg_tile).
//
// Row blocks (ccp_grid_mg_conjugate_gradient_rowblocked, ccp_grid_mg.hip) run the same kernels on levels that hold the
// block's own rows [lo, hi) plus ghost rows (MgLevel::y0, lo, hi): a tile pass covers the owned rows and reads its halo
// from the ghost rows; the restriction and the coarsening skip children outside the owned rows, so a coarse level every
// rank holds whole is the all-reduced sum of the ranks' shares.
#pragma once

#include "ccp_cg.hpp"
#include "ccp_grid_mg_view.hpp"
#include "ccp_grid_stencil.hpp"

namespace ccp {

enum MgKind { kMgSolve = 0, kMgMasked = 1, kMgCoarse = 2 };

constexpr int kMgTailSide = 32;                                   // tail: levels >= 1 with W, H <= 32
constexpr int kMgTailLevels = 6;                                  // 32, 16, 8, 4, 2, 1
constexpr int kMgTailCells = 32 * 32 + 16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1;
constexpr int kMgTileW = 64, kMgTileH = 32;                       // output tile of k_mg_tile (halo 2 nu around it)

__host__ __device__ constexpr int mg_tile_lds(int nu)
{
    return 2 * (kMgTileW + 4 * nu) * (kMgTileH + 4 * nu) * (int)sizeof(double);   // b and z of the tile and its halo
}

// A level's buffers hold local rows [0, H) of its global level: global row y0 + y at local row y.  The rows the
// level owns are [lo, hi); the others are ghost rows filled from the neighbouring row blocks.  One block, or a level
// every rank holds whole: y0 = 0, lo = 0, hi = H.  y0 is even, so (x + y) & 1 is the global colour of local cell (x, y).
struct MgLevel {
    int W, H;                         // W: the level's width; H: local rows in the buffers
    long pitch;
    const double *d, *we, *ws;        // coarse levels (level 0 derives its operator from g0 / mask)
    const unsigned char *mask;        // level 0 of a Dirichlet-mask grid
    Geom g0;                          // level 0: the global image (W, H) and the buffers' local_rows
    int y0, lo, hi;                   // global row of local row 0; owned local rows
};

__host__ __device__ __forceinline__ long mg_at(long pitch, int x, int y)
{
    return ((long)y * 2 + ((x + y) & 1)) * pitch + (x >> 1);
}

__device__ __forceinline__ double mg_ld(const double *__restrict__ v, const MgLevel &lv, int x, int y)
{
    return (x >= 0 && x < lv.W && y >= 0 && y < lv.H) ? v[mg_at(lv.pitch, x, y)] : 0.0;
}

// ---- the per-cell formulas ---------------------------------------------------------------------------------------------
// Each is written once, for T = double (this file, ccp_grid_mgb.hpp) and T = float (ccp_grid_mgs.hpp); level 0 of
// SolveChannel's matrix uses gs_update / apply_row (ccp_grid_stencil.hpp) the same way.  The callers differ only in where
// the operands come from (global memory, LDS, registers) and load them themselves; a missing neighbour is passed as 0.

// the stored operator's neighbour sum: weight and value of the north, west, east and south neighbour, in this order
template <typename T>
__device__ __forceinline__ T mg_nb_sum(T wn, T xu, T ww, T xl, T we, T xr, T ws, T xd)
{
    T s = T(0);
    s += wn * xu;
    s += ww * xl;
    s += we * xr;
    s += ws * xd;
    return s;
}

// Gauss-Seidel update and residual of a live cell of a stored operator, s its mg_nb_sum (the division is IEEE)
template <typename T>
__device__ __forceinline__ T mg_stored_update(T b, T s, T d) { return (b + s) / d; }

template <typename T>
__device__ __forceinline__ T mg_stored_residual(T b, T d, T xi, T s) { return b - (d * xi - s); }

// a live cell of the Dirichlet-mask Laplacian: k_half_sweep's masked arithmetic, b - sigma with
// sigma = (((-xu) + (-xl)) + (-xr)) + (-xd) and a_ii = 4; and its row of A x in applyToVector's order
template <typename T>
__device__ __forceinline__ T mg_masked_update(T b, T xu, T xl, T xr, T xd) { return (b + (((xu + xl) + xr) + xd)) * T(0.25); }

template <typename T>
__device__ __forceinline__ T mg_masked_row(T xi, T xu, T xl, T xr, T xd)
{
    T ax = T(0);
    ax += T(-1) * xu;
    ax += T(-1) * xl;
    ax += T(4) * xi;
    ax += T(-1) * xr;
    ax += T(-1) * xd;
    return ax;
}

template <int KIND>
__device__ __forceinline__ bool mg_live(const MgLevel &lv, int x, int y)
{
    if (KIND == kMgSolve) return classify(lv.g0, x, lv.y0 + y, y).diag != 0;
    if (KIND == kMgMasked) return lv.mask[mg_at(lv.pitch, x, y)] != 0;
    return lv.d[mg_at(lv.pitch, x, y)] != 0.0;
}

// the operator's coefficients of (x,y): 0 outside the level's owned rows and on dead pixels
template <int KIND>
__device__ __forceinline__ void mg_coef(const MgLevel &lv, int x, int y, double &d, double &we, double &ws)
{
    d = we = ws = 0.0;
    if (x >= lv.W || y < lv.lo || y >= lv.hi) return;
    const long at = mg_at(lv.pitch, x, y);
    if (KIND == kMgSolve) {
        const Stencil s = classify(lv.g0, x, lv.y0 + y, y);
        d = (double)s.diag;
        we = s.right ? 1.0 : 0.0;
        ws = s.down ? 1.0 : 0.0;
    } else if (KIND == kMgMasked) {
        if (!lv.mask[at]) return;
        d = 4.0;
        we = (x + 1 < lv.W && lv.mask[mg_at(lv.pitch, x + 1, y)]) ? 1.0 : 0.0;
        ws = (y + 1 < lv.H && lv.mask[mg_at(lv.pitch, x, y + 1)]) ? 1.0 : 0.0;
    } else {
        d = lv.d[at];
        we = lv.we[at];
        ws = lv.ws[at];
    }
}

// one Gauss-Seidel update of (x,y) from b and the four neighbours' values (0.0 outside the level)
template <int KIND>
__device__ __forceinline__ double mg_update(const MgLevel &lv, double bv, double xu, double xl, double xr, double xd, int x, int y)
{
    const long at = mg_at(lv.pitch, x, y);
    if (KIND == kMgSolve) {
        double out = 0.0;
        return gs_update(classify(lv.g0, x, lv.y0 + y, y), bv, xu, xl, xr, xd, out) ? out : 0.0;
    } else if (KIND == kMgMasked) {
        return lv.mask[at] ? mg_masked_update(bv, xu, xl, xr, xd) : 0.0;
    } else {
        const double d = lv.d[at];
        if (d == 0.0) return 0.0;
        const double s = mg_nb_sum(mg_ld(lv.ws, lv, x, y - 1), xu, mg_ld(lv.we, lv, x - 1, y), xl, lv.we[at], xr, lv.ws[at], xd);
        return mg_stored_update(bv, s, d);
    }
}

// (A z)(x,y) on level 0 in applyToVector's order (k_apply's rows); 0 on dead pixels
template <int KIND>
__device__ __forceinline__ double mg_row0(const MgLevel &lv, const double *__restrict__ z, int x, int y)
{
    const long at = mg_at(lv.pitch, x, y);
    const double xi = z[at];
    const double xu = mg_ld(z, lv, x, y - 1), xl = mg_ld(z, lv, x - 1, y), xr = mg_ld(z, lv, x + 1, y), xd = mg_ld(z, lv, x, y + 1);
    if (KIND == kMgSolve) return apply_row(classify(lv.g0, x, lv.y0 + y, y), xi, xu, xl, xr, xd);
    if (KIND == kMgCoarse) return weighted_row(lv.d, lv.we, lv.ws, lv.pitch, lv.W, lv.H, z, x, y);   // a weighted handle's level 0
    return lv.mask[at] ? mg_masked_row(xi, xu, xl, xr, xd) : 0.0;
}

// b - A z at (x,y); 0 outside the level's owned rows and on dead pixels
template <int KIND>
__device__ __forceinline__ double mg_residual(const MgLevel &lv, const double *__restrict__ b, const double *__restrict__ z, int x, int y)
{
    if (x >= lv.W || y < lv.lo || y >= lv.hi) return 0.0;
    const long at = mg_at(lv.pitch, x, y);
    if constexpr (KIND != kMgCoarse) {
        return mg_live<KIND>(lv, x, y) ? b[at] - mg_row0<KIND>(lv, z, x, y) : 0.0;
    } else {
        const double d = lv.d[at];
        if (d == 0.0) return 0.0;
        const double xi = z[at];
        const double xu = mg_ld(z, lv, x, y - 1), xl = mg_ld(z, lv, x - 1, y), xr = mg_ld(z, lv, x + 1, y), xd = mg_ld(z, lv, x, y + 1);
        const double s = mg_nb_sum(mg_ld(lv.ws, lv, x, y - 1), xu, mg_ld(lv.we, lv, x - 1, y), xl, lv.we[at], xr, lv.ws[at], xd);
        return mg_stored_residual(b[at], d, xi, s);
    }
}

// out := A in on level 0's owned rows (the PCG's products).  grid = (ceil(ceil(W/2)/kBlock), rows, 2): a thread owns
// half-column j of colour blockIdx.z in rows lo + blockIdx.y, lo + blockIdx.y + gridDim.y, ...; the caller sizes gridDim.y so that the whole grid has
// ~2,048 blocks.  DOT: one partial sum of in'(A in) per block at [(z * gridDim.y + y) * gridDim.x + x].  A no-op once the
// PCG loop has stopped (st may be null: always run).
template <int KIND, bool DOT>
__global__ void __launch_bounds__(kBlock)
k_mg_apply(MgLevel lv, const double *__restrict__ in, double *__restrict__ out, double *__restrict__ partial,
           const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    if (st && !st->active) return;                                   // (uniform)
    const int j = blockIdx.x * kBlock + threadIdx.x, c = blockIdx.z;
    double dot = 0.0;
    for (int y = lv.lo + blockIdx.y; y < lv.hi; y += gridDim.y) {
        const int x = 2 * j + ((y + c) & 1);
        if (x < lv.W) {
            const long at = mg_at(lv.pitch, x, y);
            const double ax = mg_row0<KIND>(lv, in, x, y);
            out[at] = ax;
            dot += in[at] * ax;
        }
    }
    if (DOT) {
        const double t = block_sum(dot, scratch);
        if (threadIdx.x == 0) partial[((long)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// ---- hierarchy ------------------------------------------------------------------------------------------------------
// coarse cell (X,Y) of level k+1 from level k: d = sum of the live children's diagonals - 2 x their internal edges,
// we / ws = the weights of the edges that leave the aggregate eastward / southward.  Children outside the fine level's
// owned rows count as dead: a row block adds its share of an aggregate split across two blocks, and the shares are
// summed over the ranks.  grid = (ceil(Wc/kBlock), coarse rows from local row Y0).
template <int KIND>
__global__ void __launch_bounds__(kBlock)
k_mg_coarsen(MgLevel lv, MgLevel cv, int Y0, double *__restrict__ d, double *__restrict__ we, double *__restrict__ ws)
{
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = Y0 + (int)blockIdx.y;
    if (X >= cv.W) return;
    const int x = 2 * X, y = 2 * (cv.y0 + Y) - lv.y0;
    double d00, e00, s00, d10, e10, s10, d01, e01, s01, d11, e11, s11;
    mg_coef<KIND>(lv, x, y, d00, e00, s00);
    mg_coef<KIND>(lv, x + 1, y, d10, e10, s10);
    mg_coef<KIND>(lv, x, y + 1, d01, e01, s01);
    mg_coef<KIND>(lv, x + 1, y + 1, d11, e11, s11);
    // (a weight is non-zero only between two live pixels, and 0 towards anything outside the level)
    const long at = mg_at(cv.pitch, X, Y);
    d[at] = ((d00 + d10) + (d01 + d11)) - 2.0 * ((e00 + e01) + (s00 + s10));
    we[at] = e10 + e11;
    ws[at] = s01 + s11;
}

// Weighted hierarchies: coarse cell (X,Y) of level k+1 from level k and its data weights lam (one block, whole levels):
// lambda_c = (l00 + l10) + (l01 + l11); d = lambda_c; d += north; d += west; d += east; d += south, each side the sum
// of the two fine edge weights that leave the aggregate there (north: the ws of the row above, left child first; west:
// the we of the column to the left, upper child first); we / ws as k_mg_coarsen forms them.  Every term is >= 0, so a
// coarse diagonal is never a difference.  `edge` (uniform) scales the four side sums: 1.0 for the Galerkin hierarchy,
// 0.5 for the rescaled one (CCP_MG_HIERARCHY_RESCALED), whose correction is then added unscaled; both products are
// exact, and lambda_c takes no factor.
__device__ __forceinline__ void mg_coarsen_weighted_cell(const MgLevel &lv, const double *__restrict__ lam, const MgLevel &cv, int X, int Y,
                                                         double *__restrict__ d, double *__restrict__ we, double *__restrict__ ws,
                                                         double *__restrict__ lam_c, double edge)
{
    const int x = 2 * X, y = 2 * Y;
    const double lc = (mg_ld(lam, lv, x, y) + mg_ld(lam, lv, x + 1, y)) + (mg_ld(lam, lv, x, y + 1) + mg_ld(lam, lv, x + 1, y + 1));
    const double n = edge * (mg_ld(lv.ws, lv, x, y - 1) + mg_ld(lv.ws, lv, x + 1, y - 1));
    const double w = edge * (mg_ld(lv.we, lv, x - 1, y) + mg_ld(lv.we, lv, x - 1, y + 1));
    const double e = edge * (mg_ld(lv.we, lv, x + 1, y) + mg_ld(lv.we, lv, x + 1, y + 1));
    const double s = edge * (mg_ld(lv.ws, lv, x, y + 1) + mg_ld(lv.ws, lv, x + 1, y + 1));
    double dc = lc;
    dc += n;
    dc += w;
    dc += e;
    dc += s;
    const long at = mg_at(cv.pitch, X, Y);
    d[at] = dc;
    we[at] = e;
    ws[at] = s;
    lam_c[at] = lc;
}

// level 0's coefficients in the level layout (ccp_grid_mg_level only).  grid = (ceil(W/kBlock), H).
template <int KIND>
__global__ void __launch_bounds__(kBlock)
k_mg_coef0(MgLevel lv, double *__restrict__ d, double *__restrict__ we, double *__restrict__ ws)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x >= lv.W) return;
    const long at = mg_at(lv.pitch, x, y);
    mg_coef<KIND>(lv, x, y, d[at], we[at], ws[at]);
}

// ---- one level of the V-cycle (levels above the tail) -----------------------------------------------------------------
// Every kernel does nothing once the PCG loop has stopped (st->active == 0; st may be null: always run).

// residual of the four children of coarse cell (X,Y), added up into the coarse right-hand side (children outside the
// fine level's owned rows give 0, as in k_mg_coarsen).  grid = (ceil(Wc/kBlock), coarse rows from local row Y0).
template <int KIND>
__global__ void __launch_bounds__(kBlock)
k_mg_restrict(MgLevel lv, const double *__restrict__ b, const double *__restrict__ z, MgLevel cv, int Y0, double *__restrict__ bc,
              const CgState *__restrict__ st)
{
    if (st && !st->active) return;
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = Y0 + (int)blockIdx.y;
    if (X >= cv.W) return;
    const int x = 2 * X, y = 2 * (cv.y0 + Y) - lv.y0;
    const double r00 = mg_residual<KIND>(lv, b, z, x, y), r10 = mg_residual<KIND>(lv, b, z, x + 1, y);
    const double r01 = mg_residual<KIND>(lv, b, z, x, y + 1), r11 = mg_residual<KIND>(lv, b, z, x + 1, y + 1);
    bc[mg_at(cv.pitch, X, Y)] = (r00 + r10) + (r01 + r11);
}

// All nu pre-smoothing sweeps from z = 0 (POST = false: red, black), or the prolongation z += cs * e_c on live pixels and
// all nu post-smoothing sweeps (POST = true: black, red), in ONE pass: a workgroup owns a kMgTileW x kMgTileH tile of the
// level, loads b (and z, e_c) of the tile plus a halo of 2 nu cells on every side into LDS, runs the 2 nu half-sweeps
// there and stores the tile.  A halo cell next to the edge of the LDS region sees 0.0 for its missing neighbour; the
// error moves inwards one cell per half-sweep, so after 2 nu half-sweeps the tile itself holds exactly the values the
// sweeps over the whole level give.  Bytes per cell of the tile: pre-smoothing b 8 x halo factor + z 8; post-smoothing
// (b, z 16 + e_c 2) x halo factor + z 8 (halo factor (64 + 4 nu)(32 + 4 nu) / (64 x 32): 1.41 at nu = 2).
// z_in and z_out must be different buffers: the halo of a tile is read while the neighbouring workgroups store theirs
// (pre-smoothing reads no z at all).  On a row block the tiles cover the owned rows and the halo reads the ghost rows,
// which must hold the neighbours' b (and z_in) for 2 nu rows; cells beyond them are further than 2 nu from an owned
// row, and only owned rows are stored.  grid = (ceil(W / kMgTileW), ceil((hi - lo) / kMgTileH)); dynamic LDS
// mg_tile_lds(nu) bytes.
template <int KIND, bool POST>
__global__ void __launch_bounds__(kBlock)
k_mg_tile(MgLevel lv, const double *__restrict__ b, const double *__restrict__ z_in, double *__restrict__ z_out, MgLevel cv,
          const double *__restrict__ ec, double cs, int nu, const CgState *__restrict__ st)
{
    extern __shared__ double tile_lds[];
    if (st && !st->active) return;                                   // (uniform)
    const int h = 2 * nu, RW = kMgTileW + 2 * h, RH = kMgTileH + 2 * h, n = RW * RH;
    double *sb = tile_lds, *sz = tile_lds + n;
    const int x0 = blockIdx.x * kMgTileW - h, y0 = lv.lo + blockIdx.y * kMgTileH - h;   // x0 even: a cell's x parity is its column's
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const int x = x0 + i % RW, y = y0 + i / RW;
        double bv = 0.0, zv = 0.0;                                   // outside the level: 0.0, never updated
        if (x >= 0 && x < lv.W && y >= 0 && y < lv.H) {
            const long at = mg_at(lv.pitch, x, y);
            bv = b[at];
            if (POST) {
                zv = z_in[at];
                if (mg_live<KIND>(lv, x, y)) zv = zv + cs * ec[mg_at(cv.pitch, x >> 1, ((lv.y0 + y) >> 1) - cv.y0)];   // (cs * e_c is exact)
            }
        }
        sb[i] = bv;
        sz[i] = zv;
    }
    __syncthreads();
    const int hw = RW / 2;
    auto half_sweep = [&](int c) {
        for (int k = threadIdx.x; k < hw * RH; k += kBlock) {
            const int r = k / hw, y = y0 + r;
            const int col = 2 * (k % hw) + ((c + y) & 1), x = x0 + col;
            if (x < 0 || x >= lv.W || y < 0 || y >= lv.H) continue;
            const int i = r * RW + col;
            const double xu = r > 0 ? sz[i - RW] : 0.0, xd = r + 1 < RH ? sz[i + RW] : 0.0;
            const double xl = col > 0 ? sz[i - 1] : 0.0, xr = col + 1 < RW ? sz[i + 1] : 0.0;
            sz[i] = mg_update<KIND>(lv, sb[i], xu, xl, xr, xd, x, y);
        }
        __syncthreads();
    };
    for (int s = 0; s < nu; ++s) {
        half_sweep(POST ? 1 : 0);
        half_sweep(POST ? 0 : 1);
    }
    for (int i = threadIdx.x; i < kMgTileW * kMgTileH; i += kBlock) {
        const int col = h + i % kMgTileW, r = h + i / kMgTileW, x = x0 + col, y = y0 + r;
        if (x < lv.W && y < lv.hi) z_out[mg_at(lv.pitch, x, y)] = sz[r * RW + col];
    }
}

// ---- the tail: every level from `first` down to 1x1 in one workgroup, resident in LDS --------------------------------
template <typename T>
struct MgTailT {
    int levels;
    int W[kMgTailLevels], H[kMgTailLevels], off[kMgTailLevels];   // off: first cell of the level in the LDS arrays (raster order)
    long pitch[kMgTailLevels];
    const T *d[kMgTailLevels], *we[kMgTailLevels], *ws[kMgTailLevels];
};
using MgTail = MgTailT<double>;

// The tail's V-cycle, the whole workgroup's work.  b_top: right-hand side of the tail's first level (its level layout);
// z_top: its correction; cs: the correction scale (2.0 or 1.0, as k_mg_tile's).  Three kernels instantiate it: k_mg_tail
// (below), k_mgb_tail (ccp_grid_mgb.hpp: one workgroup per channel, b_top and z_top offset to the channel) and
// k_mgs_tail (ccp_grid_mgs.hpp: T = float).
template <typename T>
__device__ __forceinline__ void mg_tail_body(const MgTailT<T> &t, const T *__restrict__ b_top, T *__restrict__ z_top, T cs, int nu)
{
    __shared__ T sd[kMgTailCells], swe[kMgTailCells], sws[kMgTailCells], sb[kMgTailCells], sz[kMgTailCells];
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
    // the coarse-level arithmetic of mg_update / mg_residual on the LDS copy
    auto sum_nb = [&](int k, int X, int Y, T &xi) -> T {
        const int W = t.W[k], H = t.H[k], o = t.off[k], i = o + Y * W + X;
        xi = sz[i];
        return mg_nb_sum(Y > 0 ? sws[i - W] : T(0), Y > 0 ? sz[i - W] : T(0), X > 0 ? swe[i - 1] : T(0), X > 0 ? sz[i - 1] : T(0),
                         swe[i], X + 1 < W ? sz[i + 1] : T(0), sws[i], Y + 1 < H ? sz[i + W] : T(0));
    };
    auto sweep = [&](int k, int c, bool first) {
        const int W = t.W[k], n = t.W[k] * t.H[k], o = t.off[k];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int X = i % W, Y = i / W;
            if (((X + Y) & 1) != c) continue;
            const T d = sd[o + i];
            T v = T(0);
            if (d != T(0)) {
                T xi;
                const T s = first ? T(0) : sum_nb(k, X, Y, xi);
                v = mg_stored_update(sb[o + i], s, d);
            }
            sz[o + i] = v;
        }
        __syncthreads();
    };
    auto residual = [&](int k, int X, int Y) -> T {
        if (X >= t.W[k] || Y >= t.H[k]) return T(0);
        const int i = t.off[k] + Y * t.W[k] + X;
        const T d = sd[i];
        if (d == T(0)) return T(0);
        T xi;
        const T s = sum_nb(k, X, Y, xi);
        return mg_stored_residual(sb[i], d, xi, s);
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
            const T r00 = residual(k, 2 * X, 2 * Y), r10 = residual(k, 2 * X + 1, 2 * Y);
            const T r01 = residual(k, 2 * X, 2 * Y + 1), r11 = residual(k, 2 * X + 1, 2 * Y + 1);
            sb[oc + i] = (r00 + r10) + (r01 + r11);
        }
        __syncthreads();
    }
    {
        const int n = t.W[last] * t.H[last], o = t.off[last];
        for (int i = threadIdx.x; i < n; i += kBlock) sz[o + i] = sd[o + i] != T(0) ? sb[o + i] / sd[o + i] : T(0);
        __syncthreads();
    }
    for (int k = last - 1; k >= 0; --k) {
        const int W = t.W[k], n = t.W[k] * t.H[k], o = t.off[k], Wc = t.W[k + 1], oc = t.off[k + 1];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int X = i % W, Y = i / W;
            if (sd[o + i] != T(0)) sz[o + i] = sz[o + i] + cs * sz[oc + (Y >> 1) * Wc + (X >> 1)];
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

// grid = 1 workgroup
static __global__ void __launch_bounds__(kBlock)
k_mg_tail(MgTail t, const double *__restrict__ b_top, double *__restrict__ z_top, double cs, int nu, const CgState *__restrict__ st)
{
    if (st && !st->active) return;
    mg_tail_body(t, b_top, z_top, cs, nu);
}

// ---- PCG scalars (the vector passes are ccp_cg.hpp's: k_cg_update, k_cg_dot, k_cg_direction) -------------------------
// The two steps (thread 0 stores), for k_mg_check / k_mg_beta and, per channel, k_mgb_check / k_mgb_beta (ccp_grid_mgb.hpp).
// rr = r'r of the update just made: `if (sqrt(r'r) < epsilon) break;` before the V-cycle of the next direction runs
__device__ __forceinline__ void mg_check_step(double rr, double epsilon, CgState *__restrict__ st)
{
    if (threadIdx.x == 0 && st->active) {
        st->r1norm = sqrt(rr);
        if (st->r1norm < epsilon) {
            st->active = 0;
            st->converged = 1;
        }
    }
}

// beta = new r'z / old r'z; ++iterations (k_pcg_beta's count)
__device__ __forceinline__ void mg_beta_step(double rz, CgState *__restrict__ st)
{
    if (threadIdx.x == 0 && st->active) {
        st->beta = rz / st->rlen;
        st->rlen = rz;
        st->iterations += 1;
    }
}

static __global__ void __launch_bounds__(kBlock)
k_mg_check(const double *__restrict__ partial, int count, double epsilon, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mg_check_step(reduce_partials(partial, count, scratch), epsilon, st);
}

static __global__ void __launch_bounds__(kBlock)
k_mg_beta(const double *__restrict__ partial, int count, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mg_beta_step(reduce_partials(partial, count, scratch), st);
}

}  // namespace ccp
