// ccp_grid_mgn.hpp — CCP_MG_NULLSPACE_CONSTANT (include/ccp_gs.h): the multigrid PCG of a weighted handle whose operator
// is floating (lambda = 0 everywhere, no fixed pixel, every in-canvas edge weight > 0: the constants are its null space),
// hand-written for gfx950.  The loop and its operation order are in the header; the V-cycle, the product and the update
// pass are the NONE loop's own kernels (ccp_grid_mg.hpp, ccp_cg.hpp).  What is here:
//
//   k_mgn_census     is every operator of the handle floating?  Once per installed operator.
//   k_mgn_dot        the reduction variant: k_cg_dot's read of r and z also yields sum(z) and sum(r)
//   k_mgn_rz         the one-block step after it: zm = sum(z) / n, r'z - zm sum(r) as the new r'z (and beta), zm kept as a
//                    device scalar (MgnState)
//   k_mgn_direction  the direction variant: p = (z - zm) + beta p, zm read from the device scalar
//   k_mgn_sums, k_mgn_means, k_mgn_init, k_mgn_center, k_mgn_shift
//                    once per solve: bm = mean(b), m0 = mean(x), r = (b - bm) - A x, and the closing x += m0 - mean(x)
//
// Layout.  The vectors are one channel of the handle's colour-split layout (mg_at): row y has two planes of `pitch`
// doubles, plane (x + y) & 1 first-indexed by x >> 1; ch_stride = 2 H pitch.  The cells beyond ceil(W/2) or floor(W/2)
// of a plane are padding: zero in every vector, never written.  A pass that adds a constant to a vector (k_mgn_init,
// k_mgn_center, k_mgn_direction, k_mgn_shift) or sums a caller's vector (k_mgn_sums) therefore visits the pixels only
// (mgn_for_pixels); k_mgn_dot sums r and z over the whole range as k_cg_dot does: their padding is zero.
// A floating operator has no dead pixel (the census asks for d > 0 too, which refuses the 1x1 canvas), so none of the
// passes looks at d.
//
// Sums: wave shuffles and a fixed order over the waves and the blocks (block_sum, reduce_partials of ccp_common.hpp /
// ccp_cg.hpp): deterministic, the same bits on every run.
#pragma once

#include "ccp_grid_mg.hpp"

namespace ccp {

// one channel's layout: W pixels per row, 2 H plane rows of `pitch` doubles
struct MgnLay {
    int W, rows2, pitch;
};

// the device scalars of one solve beside CgState
struct MgnState {
    double b_mean;       // mean(b)
    double m0;           // mean(x) on entry
    double z_mean;       // mean(z) of the V-cycle just run
    double shift;        // the closing m0 - mean(x)
    double x_mean;       // mean(x) as returned
};

enum MgnMean { kMgnStart = 0, kMgnClose = 1, kMgnReport = 2 };

// f(i) for every pixel i of k_cg_*'s grid-stride range of this thread (index i of the layout; padding skipped).  The
// plane row and the half-column are carried along instead of divided out per element.
template <typename F>
__device__ __forceinline__ void mgn_for_pixels(const MgnLay &l, F &&f)
{
    const long n = (long)l.rows2 * l.pitch;
    const long first = (long)blockIdx.x * kBlock + threadIdx.x, stride = (long)gridDim.x * kBlock;
    if (first >= n) return;
    int row = (int)(first / l.pitch), hc = (int)(first - (long)row * l.pitch);
    const int srow = (int)(stride / l.pitch), shc = (int)(stride - (long)srow * l.pitch);
    for (long i = first; i < n; i += stride) {
        const int x = 2 * hc + (((row & 1) + (row >> 1)) & 1);       // plane c of row y holds the x with (x + y) & 1 == c
        if (x < l.W) f(i);
        row += srow;
        hc += shc;
        if (hc >= l.pitch) {
            hc -= l.pitch;
            ++row;
        }
    }
}

// ---- the census ------------------------------------------------------------------------------------------------------
// count[set] += the pixels of operator `set` that keep it from floating: lambda != 0 (a screened pixel, or the -1 that
// marks a fixed one), an east edge inside the canvas whose weight is not > 0, a south edge likewise, or d not > 0 (a 1x1
// canvas, which has no edge: its operator is 0).  Set k's d, we, ws, lambda planes: op + k * op_stride, `plane` doubles
// apart.  grid = (ceil(W/kBlock), H, sets); count zeroed by the caller.
static __global__ void __launch_bounds__(kBlock)
k_mgn_census(const double *__restrict__ op, long op_stride, long plane, int W, int H, long pitch, unsigned *__restrict__ count)
{
    __shared__ unsigned bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x < W) {
        const double *__restrict__ o = op + (long)blockIdx.z * op_stride;
        const long at = mg_at(pitch, x, y);
        const bool ok = o[at] > 0.0 && o[3 * plane + at] == 0.0 && (x + 1 >= W || o[plane + at] > 0.0) && (y + 1 >= H || o[2 * plane + at] > 0.0);
        if (!ok) atomicAdd(&bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad) atomicAdd(&count[blockIdx.z], bad);
}

// ---- once per solve --------------------------------------------------------------------------------------------------
// partial[blockIdx.x] = this block's share of sum(a), partial[gridDim.x + blockIdx.x] = of sum(b) (b may be null: 0)
static __global__ void __launch_bounds__(kBlock)
k_mgn_sums(const double *__restrict__ a, const double *__restrict__ b, MgnLay l, double *__restrict__ partial)
{
    __shared__ double scratch[kBlock / kWave];
    double sa = 0.0, sb = 0.0;
    mgn_for_pixels(l, [&](long i) {
        sa += a[i];
        if (b) sb += b[i];
    });
    const double ta = block_sum(sa, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = ta;
    const double tb = block_sum(sb, scratch);
    if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = tb;
}

// one block, after k_mgn_sums left `count` partials of each sum; n = W H as a double.  kMgnStart: b_mean = sum0 / n,
// m0 = sum1 / n.  kMgnClose: shift = m0 - sum0 / n.  kMgnReport: x_mean = sum0 / n.
// hold (the enqueue solve: the operator's status word; null otherwise): while it is non-zero the solve never
// started and must leave x alone bit for bit, so kMgnClose stores -0.0, the one shift k_mgn_shift's x + shift returns
// every x unchanged for (+0.0 would turn a -0.0 of x into +0.0).
static __global__ void __launch_bounds__(kBlock)
k_mgn_means(const double *__restrict__ partial, int count, double n, int which, MgnState *__restrict__ ns, const unsigned *__restrict__ hold)
{
    __shared__ double scratch[kBlock / kWave];
    const double s0 = reduce_partials(partial, count, scratch);
    const double s1 = reduce_partials(partial + count, count, scratch);
    if (threadIdx.x != 0) return;
    if (which == kMgnStart) {
        ns->b_mean = s0 / n;
        ns->m0 = s1 / n;
    } else if (which == kMgnClose) {
        ns->shift = hold && *hold ? -0.0 : ns->m0 - s0 / n;
    } else {
        ns->x_mean = s0 / n;
    }
}

// r := (b - bm) - r on the pixels (r holds A x on entry); the thread's share of r'r into partial[blockIdx.x]
static __global__ void __launch_bounds__(kBlock)
k_mgn_init(const double *__restrict__ b, double *__restrict__ r, MgnLay l, const MgnState *__restrict__ ns, double *__restrict__ partial)
{
    __shared__ double scratch[kBlock / kWave];
    const double bm = ns->b_mean;
    double acc = 0.0;
    mgn_for_pixels(l, [&](long i) {
        const double v = (b[i] - bm) - r[i];
        r[i] = v;
        acc += v * v;
    });
    const double t = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// out := b - bm on the pixels (ccp_grid_mg_apply's right-hand side; out's padding is zero and stays so)
static __global__ void __launch_bounds__(kBlock)
k_mgn_center(const double *__restrict__ b, double *__restrict__ out, MgnLay l, const MgnState *__restrict__ ns)
{
    const double bm = ns->b_mean;
    mgn_for_pixels(l, [&](long i) { out[i] = b[i] - bm; });
}

// x += shift on the pixels
static __global__ void __launch_bounds__(kBlock)
k_mgn_shift(double *__restrict__ x, MgnLay l, const MgnState *__restrict__ ns)
{
    const double shift = ns->shift;
    mgn_for_pixels(l, [&](long i) { x[i] = x[i] + shift; });
}

// ---- once per iteration ----------------------------------------------------------------------------------------------
// The reduction variant of k_cg_dot: the block's shares of r'z, sum(z) and sum(r) from one read of r and z, at
// partial[blockIdx.x], partial[gridDim.x + blockIdx.x], partial[2 gridDim.x + blockIdx.x].  A no-op on the vectors once
// the loop has stopped (zeros are stored, as k_cg_dot does).
static __global__ void __launch_bounds__(kBlock)
k_mgn_dot(const double *__restrict__ r, const double *__restrict__ z, long n, double *__restrict__ partial, const CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    double rz = 0.0, sz = 0.0, sr = 0.0;
    if (st->active)
        for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
            const double rv = r[i], zv = z[i];
            rz += rv * zv;
            sz += zv;
            sr += rv;
        }
    const double t0 = block_sum(rz, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = t0;
    const double t1 = block_sum(sz, scratch);
    if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = t1;
    const double t2 = block_sum(sr, scratch);
    if (threadIdx.x == 0) partial[2 * gridDim.x + blockIdx.x] = t2;
}

// one block: zm = sum(z) / n, rz = r'z - zm sum(r); FIRST: rlen = rz (k_cg_set_rlen's step), otherwise k_mg_beta's step
// with it.  zm goes to ns->z_mean for k_mgn_direction.
template <bool FIRST>
static __global__ void __launch_bounds__(kBlock)
k_mgn_rz(const double *__restrict__ partial, int count, double n, CgState *__restrict__ st, MgnState *__restrict__ ns)
{
    __shared__ double scratch[kBlock / kWave];
    const double rz = reduce_partials(partial, count, scratch);
    const double sz = reduce_partials(partial + count, count, scratch);
    const double sr = reduce_partials(partial + 2 * count, count, scratch);
    const double zm = sz / n;
    const double v = rz - zm * sr;
    if (threadIdx.x == 0 && st->active) ns->z_mean = zm;
    if (FIRST) cg_set_rlen_step(v, st);
    else mg_beta_step(v, st);
}

// The direction variant of k_cg_direction: p := (z - zm) + beta p on the pixels; FIRST: p := z - zm.
template <bool FIRST>
static __global__ void __launch_bounds__(kBlock)
k_mgn_direction(double *__restrict__ p, const double *__restrict__ z, MgnLay l, const CgState *__restrict__ st, const MgnState *__restrict__ ns)
{
    if (!st->active) return;
    const double zm = ns->z_mean, beta = FIRST ? 0.0 : st->beta;
    mgn_for_pixels(l, [&](long i) {
        const double v = z[i] - zm;
        p[i] = FIRST ? v : v + beta * p[i];
    });
}

}  // namespace ccp
