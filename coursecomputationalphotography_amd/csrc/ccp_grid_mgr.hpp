// ccp_grid_mgr.hpp — the kernels of the enqueue-only multigrid PCG whose stop test is relative to |b| (include/ccp_gs.h:
// ccp_grid_mg_conjugate_gradient_enqueue_relative), hand-written for gfx950.  The recurrence and every other kernel are
// the absolute call's (ccp_grid_mg.hpp, ccp_cg.hpp, ccp_grid_mgb.hpp, ccp_grid_mgn.hpp, ccp_grid_mge.hpp); what differs
// is where the threshold comes from:
//
//   k_mgr_init, k_mgr_init_constant, k_mgr_init_batched
//                    the init passes k_cg_init, k_mgn_init, k_mgb_init with a second accumulator: while they read b for
//                    r = b - A x they also sum b b (CONSTANT mode: (b - bm)(b - bm)), over the same grid-stride ranges
//                    and through the same block_sum, into a second set of partial sums.  No extra pass over the image.
//   k_mgr_threshold, k_mgr_threshold_batched
//                    one workgroup (per channel): bb = reduce_partials of that second set, bnorm = sqrt(bb),
//                    eps = fmax(epsilon_abs, epsilon_rel * bnorm) -- one multiply, then fmax -- stored as device scalars
//   k_mgr_check, k_mgr_check_batched
//                    mg_check_step with the threshold read from memory and the stop rule r1norm < eps || r1norm == 0.0
//   k_mgr_report     k_mge_report's six fields, then [6] bnorm and [7] eps
//
// The first accumulator of an init pass is the absolute pass's, statement for statement: r, p and the r'r partial sums have
// its bits.  With x = 0 on entry r = b (b - 0, or (b - bm) - 0), so both accumulators add the same products in the same
// order and bb equals the initial r'r bit for bit.
// Sums: wave shuffles and a fixed order over the waves and the blocks (block_sum, reduce_partials): deterministic.
#pragma once

#include "ccp_grid_mge.hpp"

namespace ccp {

constexpr int kMgrReportFields = 8;   // k_mge_report's six, then bnorm and eps

// r := b - r, p := r over k_cg_init's range of elements [o, o + n); the thread's shares of r'r (returned) and of b'b (bb)
__device__ __forceinline__ double mgr_init_body(const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p, long o, long n,
                                                double &bb)
{
    double acc = 0.0, acc_b = 0.0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
        const double w = b[o + i];
        const double v = w - r[o + i];
        r[o + i] = v;
        p[o + i] = v;
        acc += v * v;
        acc_b += w * w;
    }
    bb = acc_b;
    return acc;
}

// k_cg_init; bpartial[blockIdx.x] = this block's share of b'b
static __global__ void __launch_bounds__(kBlock)
k_mgr_init(const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p, long n, double *__restrict__ partial,
           double *__restrict__ bpartial)
{
    __shared__ double scratch[kBlock / kWave];
    double bb = 0.0;
    const double t = block_sum(mgr_init_body(b, r, p, 0, n, bb), scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
    const double tb = block_sum(bb, scratch);
    if (threadIdx.x == 0) bpartial[blockIdx.x] = tb;
}

// k_mgb_init (grid = (the sequential pass's blocks, C)); bpartial: C slices ps apart, as partial
static __global__ void __launch_bounds__(kBlock)
k_mgr_init_batched(const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p, long n, double *__restrict__ partial,
                   double *__restrict__ bpartial, long ps)
{
    __shared__ double scratch[kBlock / kWave];
    const long o = (long)blockIdx.y * n;
    double bb = 0.0;
    const double t = block_sum(mgr_init_body(b, r, p, o, n, bb), scratch);
    if (threadIdx.x == 0) partial[blockIdx.y * ps + blockIdx.x] = t;
    const double tb = block_sum(bb, scratch);
    if (threadIdx.x == 0) bpartial[blockIdx.y * ps + blockIdx.x] = tb;
}

// k_mgn_init: r := (b - bm) - r on the pixels; bpartial[blockIdx.x] = this block's share of sum (b - bm)^2
static __global__ void __launch_bounds__(kBlock)
k_mgr_init_constant(const double *__restrict__ b, double *__restrict__ r, MgnLay l, const MgnState *__restrict__ ns, double *__restrict__ partial,
                    double *__restrict__ bpartial)
{
    __shared__ double scratch[kBlock / kWave];
    const double bm = ns->b_mean;
    double acc = 0.0, acc_b = 0.0;
    mgn_for_pixels(l, [&](long i) {
        const double w = b[i] - bm;
        const double v = w - r[i];
        r[i] = v;
        acc += v * v;
        acc_b += w * w;
    });
    const double t = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
    const double tb = block_sum(acc_b, scratch);
    if (threadIdx.x == 0) bpartial[blockIdx.x] = tb;
}

// bnorm = sqrt(bb), eps = fmax(epsilon_abs, epsilon_rel * bnorm): one multiply, then fmax (a NaN product -- 0 * inf --
// leaves epsilon_abs).  While the operator status word is non-zero (status null: never) the solve never started: both +0.0.
__device__ __forceinline__ void mgr_threshold_step(double bb, double epsilon_abs, double epsilon_rel, const unsigned *__restrict__ status,
                                                   double *__restrict__ bnorm, double *__restrict__ eps)
{
    if (threadIdx.x != 0) return;
    if (status && *status) {
        *bnorm = 0.0;
        *eps = 0.0;
        return;
    }
    const double nb = sqrt(bb);
    const double rel = epsilon_rel * nb;
    *bnorm = nb;
    *eps = fmax(epsilon_abs, rel);
}

// one workgroup, after an init pass left `count` partial sums of b'b
static __global__ void __launch_bounds__(kBlock)
k_mgr_threshold(const double *__restrict__ bpartial, int count, double epsilon_abs, double epsilon_rel, const unsigned *__restrict__ status,
                double *__restrict__ bnorm, double *__restrict__ eps)
{
    __shared__ double scratch[kBlock / kWave];
    mgr_threshold_step(reduce_partials(bpartial, count, scratch), epsilon_abs, epsilon_rel, status, bnorm, eps);
}

// one workgroup per channel: channel c's partial sums at bpartial + c ps, its scalars at bnorm[c], eps[c]
static __global__ void __launch_bounds__(kBlock)
k_mgr_threshold_batched(const double *__restrict__ bpartial, long ps, int count, double epsilon_abs, double epsilon_rel,
                        const unsigned *__restrict__ status, double *__restrict__ bnorm, double *__restrict__ eps)
{
    __shared__ double scratch[kBlock / kWave];
    mgr_threshold_step(reduce_partials(bpartial + blockIdx.x * ps, count, scratch), epsilon_abs, epsilon_rel, status, bnorm + blockIdx.x,
                       eps + blockIdx.x);
}

// mg_check_step against the channel's own threshold; a residual of exactly 0 stops too (a zero right-hand side from x = 0
// with epsilon_abs = 0: eps is 0 and 0 < 0 never holds)
__device__ __forceinline__ void mgr_check_step(double rr, const double *__restrict__ eps, CgState *__restrict__ st)
{
    if (threadIdx.x == 0 && st->active) {
        st->r1norm = sqrt(rr);
        if (st->r1norm < *eps || st->r1norm == 0.0) {
            st->active = 0;
            st->converged = 1;
        }
    }
}

static __global__ void __launch_bounds__(kBlock)
k_mgr_check(const double *__restrict__ partial, int count, const double *__restrict__ eps, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mgr_check_step(reduce_partials(partial, count, scratch), eps, st);
}

static __global__ void __launch_bounds__(kBlock)
k_mgr_check_batched(const double *__restrict__ partial, long ps, int count, const double *__restrict__ eps, CgState *__restrict__ st)
{
    __shared__ double scratch[kBlock / kWave];
    mgr_check_step(reduce_partials(partial + blockIdx.x * ps, count, scratch), eps + blockIdx.x, st + blockIdx.x);
}

// k_mge_report's row of channel c, then [6] bnorm[c] and [7] eps[c]
static __global__ void __launch_bounds__(kBlock)
k_mgr_report(const CgState *__restrict__ st, const MgnState *__restrict__ ns, int C, MgeReport out, const unsigned *__restrict__ status,
             const double *__restrict__ bnorm, const double *__restrict__ eps)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    double *__restrict__ o = out.data + c * out.stride_channel;
    o[0] = (double)st[c].iterations;
    o[out.stride_field] = st[c].converged ? 1.0 : 0.0;
    o[2 * out.stride_field] = st[c].r1norm;
    o[3 * out.stride_field] = ns ? ns[c].b_mean : 0.0;
    o[4 * out.stride_field] = ns ? ns[c].x_mean : 0.0;
    o[5 * out.stride_field] = status ? (double)*status : 0.0;
    o[6 * out.stride_field] = bnorm[c];
    o[7 * out.stride_field] = eps[c];
}

}  // namespace ccp
