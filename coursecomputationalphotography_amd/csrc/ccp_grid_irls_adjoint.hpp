// ccp_grid_irls_adjoint.hpp — ccp_grid_irls_adjoint_step_device: one step z := G + J'z of the adjoint iteration at an IRLS
// fixed point (include/ccp_gs.h, "Differentiating IRLS at its fixed point", fixes the operation order;
// tests/fixed_point_helpers.py is the same in numpy).  J'z is what one unrolled backward step forms with two passes and
// three intermediate planes -- ccp_grid_weighted_adjoint_device's g_wx, g_wy, g_lambda of (v, u), then
// ccp_grid_reweight_adjoint_device's g_u of those -- and this pass forms it in one, the upstream gradients in registers:
// they are sums over the channels of s * r with r the very residual q is summed from, at the positions u is read anyway.
// fp64 throughout, nothing contracted, every operation the two passes' own in their order: b has their bits.
//
// Geometry.  k_weighted_reweight_adjoint's (ccp_grid_reweight_adjoint.hpp): grid = (ceil(W/kBlock), ceil(H/rows), sets), a
// thread owns column x and marches down the `rows` rows of its strip.  Per row it forms its own k_x, k_y and k_d
// (irls_adjoint_k: one pass over the channels for q_x, q_y, dq AND Gwx, Gwy, Glambda).  k_N is the k_y of the row above,
// kept in a register; the strip's first row forms the k_y of (x, y0 - 1) itself.  k_W is the left lane's k_x, handed over
// through one of two LDS rows with one barrier per trip; lane 0 of a block with x >= 1 forms the k_x of (x - 1, y) itself.
// Under PIXEL coupling a neighbour's k needs both of the neighbour's forward edges, so those two reach v and u at
// (x - 1, y + 1) and (x + 1, y - 1): irls_adjoint_k guards every read with the canvas's extents, whoever asks.
//
// Report.  Every thread keeps sum (z_new - z_old)^2 and sum z_new^2 of its column's free live pixels per channel in LDS
// slots of its own (the channel count is a run-time value: registers cannot be indexed by it), the block sums them
// (block_sum: shuffles and one fixed-order loop) and thread 0 stores the block's pair; k_irls_adjoint_report sums the
// blocks' pairs of a channel, each thread its stride in order, then block_sum again.  No atomics: the same inputs give
// the same bits.
//
// Barriers.  Every __syncthreads() is reached by every thread of the block the same number of times: the trip count is the
// kernel argument `rows`, the channel count and `part` are uniform, no thread returns early, and lanes past W and rows
// past H skip the arithmetic and the stores, not the barriers.
//
// Memory.  Nothing is indexed at run time but global memory and LDS (by lane and channel slot, < 2 kMaxChannels); every
// view was checked on the host against its allocation, and the partial sums against the buffer's length.  Included by
// ccp_grid_weighted.hip alone, after ccp_grid_reweight_adjoint.hpp.
#pragma once

#include "ccp_grid_reweight_adjoint.hpp"

namespace ccp {

struct IrlsAdjointArgs {
    RobustArgs f;                // the reweight as it was described; f.dphi < 0: the plain reweight, no data term
    const double *v;             // the handle's x: the adjoint solution, channels `plane` apart (w_at)
    double *b;                   // the handle's b: z_old in, z_new out
    const double *d;             // the installed operator's d of set 0 (liveness); set k's at + k * dset
    long plane, dset;
    ImageView grad, fixed;       // G; the mask of fixed pixels (absent: none), indexed by the set
    double *part;                // the blocks' partial sums of the report; nullptr: no report
};

__device__ __forceinline__ bool irls_fixed(const IrlsAdjointArgs &a, int x, int y, int set)
{
    return a.fixed.p && a.fixed(y, x, set) != 0.0;
}

// v of channel c at (x, y): +0.0 at a fixed pixel whatever x holds there
__device__ __forceinline__ double irls_v(const IrlsAdjointArgs &a, int x, int y, int c, bool fixed)
{
    return fixed ? 0.0 : a.v[(long)c * a.plane + w_at(a.f.r.pitch, x, y)];
}

// reweight_adjoint_k with the upstream gradients formed here: k_x (want & 1), k_y (want & 2) and k_d (want & 4) of pixel
// (x, y) of set `set`; +0.0 for an absent edge or a value not asked for.  The owner asks for all of them, a neighbour for
// the one k it needs.  (x, y) is inside the canvas; every other position is read behind he / hs.
template <int PHI>
__device__ __forceinline__ void irls_adjoint_k(const IrlsAdjointArgs &a, int x, int y, int set, int want, double &kx, double &ky, double &kd)
{
    const ReweightArgs &r = a.f.r;
    const bool he = x + 1 < r.W, hs = y + 1 < r.H;
    const bool pixel = r.coupling != 0;
    const bool we = he && (want & 1), ws = hs && (want & 2), wl = (want & 4) != 0;
    const bool nx = he && (pixel ? (want & 3) != 0 : we);
    const bool ny = hs && (pixel ? (want & 3) != 0 : ws);
    const bool nd = wl && a.f.dphi != kPhiQuadratic;
    double qx = 0.0, qy = 0.0, dq = 0.0, gwx = 0.0, gwy = 0.0, gl = 0.0;
    if (nx || ny || wl) {
        const bool fc = irls_fixed(a, x, y, set);
        const bool fe = nx && irls_fixed(a, x + 1, y, set), fs = ny && irls_fixed(a, x, y + 1, set);
        const int c0 = set * r.cpb, c1 = c0 + r.cpb;
        for (int c = c0; c < c1; ++c) {
            const double u = reweight_u(r, a.plane, x, y, c);
            const double v = irls_v(a, x, y, c, fc);
            if (nx) {
                const double s = irls_v(a, x + 1, y, c, fe) - v;
                const double d = (r.gx.p ? r.gx.f32(y, x, c) : 0.0) - (reweight_u(r, a.plane, x + 1, y, c) - u);
                if (PHI != kPhiQuadratic) qx += d * d;
                gwx += s * d;
            }
            if (ny) {
                const double s = irls_v(a, x, y + 1, c, fs) - v;
                const double d = (r.gy.p ? r.gy.f32(y, x, c) : 0.0) - (reweight_u(r, a.plane, x, y + 1, c) - u);
                if (PHI != kPhiQuadratic) qy += d * d;
                gwy += s * d;
            }
            if (wl) {
                const double d = a.f.f(y, x, c) - u;
                if (nd) dq += d * d;
                if (!fc) gl += v * d;                                      // Glambda is +0.0 at a fixed pixel
            }
        }
    }
    kx = ky = kd = 0.0;
    if (pixel) {
        if (we || ws) {                                                    // one phi, one k for both forward edges
            const double q = qx + qy;
            const double p = robust_phi<PHI>(q, r.eps);
            double t = 0.0;
            if (he) t += r.bwx.p ? gwx * r.bwx(y, x, set) : gwx;
            if (hs) t += r.bwy.p ? gwy * r.bwy(y, x, set) : gwy;
            kx = ky = (t * r.scale) * reweight_psi(PHI, q, p, r.eps);
        }
    } else {
        if (we) {
            const double p = robust_phi<PHI>(qx, r.eps);
            kx = ((r.bwx.p ? gwx * r.bwx(y, x, set) : gwx) * r.scale) * reweight_psi(PHI, qx, p, r.eps);
        }
        if (ws) {
            const double p = robust_phi<PHI>(qy, r.eps);
            ky = ((r.bwy.p ? gwy * r.bwy(y, x, set) : gwy) * r.scale) * reweight_psi(PHI, qy, p, r.eps);
        }
    }
    if (wl) {
        const double p = robust_phi_data(a.f.dphi, dq, a.f.deps);
        kd = ((r.lam.p ? gl * r.lam(y, x, set) : gl) * a.f.dscale) * reweight_psi(a.f.dphi, dq, p, a.f.deps);
    }
}

// The arguments are 928 bytes, far more than a wave's scalar registers hold.  Taken as an ordinary by-value argument they
// are all fetched at the kernel's entry and kept live across the march (179 VGPRs, 176 scalar spills and, for two
// penalties, 36 bytes of scratch); read through the kernel-argument segment pointer each member is fetched by a scalar
// load where it is used (96 VGPRs, about 60 scalar spills, no scratch: NOTES R42.1).
typedef const __attribute__((address_space(4))) IrlsAdjointArgs *IrlsKernArgs;

// grid = (ceil(W/kBlock), ceil(H/a.f.rows), sets).  part: per channel c two runs of gridDim.x * gridDim.y doubles, the
// blocks' sum (z_new - z_old)^2 at (2 c) * blocks + block and sum z_new^2 at (2 c + 1) * blocks + block.
template <int PHI>
__global__ void __launch_bounds__(kBlock)
k_irls_adjoint_step(IrlsAdjointArgs)
{
    const IrlsAdjointArgs &a = *(const IrlsAdjointArgs *)(IrlsKernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ double east[2][kBlock];
    __shared__ double sums[2 * kMaxChannels][kBlock];
    __shared__ double scratch[kBlock / kWave];
    const ReweightArgs &r = a.f.r;
    const int x = blockIdx.x * kBlock + threadIdx.x, y0 = blockIdx.y * a.f.rows, ch = blockIdx.z;
    const bool column = x < r.W;
    const bool data = a.f.dphi >= 0;
    const int c0 = ch * r.cpb, c1 = c0 + r.cpb;
    const bool he = x + 1 < r.W;
    const double *d = a.d + (long)ch * a.dset;
    if (a.part)
        for (int j = 0; j < 2 * r.cpb; ++j) sums[j][threadIdx.x] = 0.0;    // the thread's own slots: no barrier needed
    double kN = 0.0;                                                       // the k_y of the row above
    if (column && y0 >= 1 && y0 < r.H) {
        double t0, t1;
        irls_adjoint_k<PHI>(a, x, y0 - 1, ch, 2, t0, kN, t1);
    }
    for (int i = 0; i < a.f.rows; ++i) {
        const int y = y0 + i;
        const bool live = column && y < r.H;
        double kx = 0.0, ky = 0.0, kd = 0.0;
        if (live) irls_adjoint_k<PHI>(a, x, y, ch, data ? 7 : 3, kx, ky, kd);
        east[i & 1][threadIdx.x] = kx;
        __syncthreads();                                                   // every thread, every trip
        if (live) {
            double kW = 0.0;
            if (threadIdx.x >= 1) {
                kW = east[i & 1][threadIdx.x - 1];
            } else if (x >= 1) {
                double t0, t1;
                irls_adjoint_k<PHI>(a, x - 1, y, ch, 1, kW, t0, t1);
            }
            const bool hs = y + 1 < r.H;
            const long at = w_at(r.pitch, x, y);
            const bool free_live = d[at] != 0.0;                           // a fixed pixel's d is 0 as a dead one's
            for (int c = c0; c < c1; ++c) {
                const double u = reweight_u(r, a.plane, x, y, c);
                double t = 0.0;
                if (he) t += kx * ((r.gx.p ? r.gx.f32(y, x, c) : 0.0) - (reweight_u(r, a.plane, x + 1, y, c) - u));
                if (hs) t += ky * ((r.gy.p ? r.gy.f32(y, x, c) : 0.0) - (reweight_u(r, a.plane, x, y + 1, c) - u));
                if (x >= 1) t -= kW * ((r.gx.p ? r.gx.f32(y, x - 1, c) : 0.0) - (u - reweight_u(r, a.plane, x - 1, y, c)));
                if (y >= 1) t -= kN * ((r.gy.p ? r.gy.f32(y - 1, x, c) : 0.0) - (u - reweight_u(r, a.plane, x, y - 1, c)));
                if (data) t -= kd * (a.f.f(y, x, c) - u);
                double *bp = a.b + (long)c * a.plane + at;
                if (free_live) {
                    const double z = a.grad(y, x, c) + t;
                    if (a.part) {
                        const double dz = z - *bp;
                        sums[2 * (c - c0)][threadIdx.x] += dz * dz;
                        sums[2 * (c - c0) + 1][threadIdx.x] += z * z;
                    }
                    *bp = z;
                } else {
                    *bp = 0.0;
                }
            }
            kN = ky;
        }
    }
    if (a.part) {                                                          // (uniform over the launch)
        const long blocks = (long)gridDim.x * gridDim.y, block = (long)blockIdx.y * gridDim.x + blockIdx.x;
        for (int j = 0; j < 2 * r.cpb; ++j) {
            const double total = block_sum(sums[j][threadIdx.x], scratch);
            if (threadIdx.x == 0) a.part[(2L * c0 + j) * blocks + block] = total;
        }
    }
}

// grid = (channels): report[c] = (sum over the blocks of part's two runs of channel c), at out + c * sy + {0, 1} * sx
__global__ void __launch_bounds__(kBlock)
k_irls_adjoint_report(const double *__restrict__ part, long blocks, double *__restrict__ out, long sy, long sx)
{
    __shared__ double scratch[kBlock / kWave];
    const int c = blockIdx.x;
    const double *__restrict__ p0 = part + (2L * c) * blocks, *__restrict__ p1 = p0 + blocks;
    double a0 = 0.0, a1 = 0.0;
    for (long i = threadIdx.x; i < blocks; i += kBlock) {
        a0 += p0[i];
        a1 += p1[i];
    }
    const double t0 = block_sum(a0, scratch);
    const double t1 = block_sum(a1, scratch);
    if (threadIdx.x == 0) {
        out[(long)c * sy] = t0;
        out[(long)c * sy + sx] = t1;
    }
}

}  // namespace ccp
