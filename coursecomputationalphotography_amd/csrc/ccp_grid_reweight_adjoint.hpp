// ccp_grid_reweight_adjoint.hpp — ccp_grid_reweight_adjoint_device: the vector-Jacobian product of the two reweight passes
// of ccp_grid_weighted.hpp (include/ccp_gs.h, "Backpropagating through a reweight", fixes the operation order;
// tests/reweight_adjoint_helpers.py is the same in numpy).  Given dL/dwx, dL/dwy (and dL/dlambda) it forms the gradients
// with respect to the u the weights were formed from, the guidance, f, and the base weights.  fp64 throughout, nothing
// contracted, only +, -, x, / and sqrt, every one correctly rounded: the outputs have the model's bits.
//
// The costly value per edge is k, the upstream gradient times d(weight)/d(q)'s factor psi: a sqrt, one or two divisions
// and the phi products, the same fp64 chain that bounds the forward passes (NOTES R38.1, R39.1).  A pixel needs four of
// them -- its own k_x, k_y and those of its west and north neighbours, whose edges end in it -- so the geometry is
// k_weighted_reweight_robust's, which forms each once:
//
// Geometry.  grid = (ceil(W/kBlock), ceil(H/rows), sets): a thread owns column x and marches down the `rows` rows of its
// strip.  Per row it forms its own k_x, k_y and k_d (reweight_adjoint_k, one pass over the channels for q_x, q_y, dq).
// k_N is the k_y it formed for the row above, kept in a register; in the strip's first row it forms the k_y of (x, y0 - 1)
// itself.  k_W is the left lane's k_x of this row: every lane writes its k_x to one of two LDS rows (east[row & 1]), one
// barrier, then reads its left neighbour's; lane 0 of a block with x >= 1 forms the k_x of (x - 1, y) itself.  Two rows
// suffice with one barrier per row, as there.  The residuals r that multiply a k are two subtractions on u values the pass
// reads anyway (its lane neighbours' and the adjacent rows' own loads: L1 / L2), so they are recomputed, not carried.
//
// Bits.  Whoever forms a k calls reweight_adjoint_k -- the same instructions on the same operands in the same order -- and a
// value that went through a register or LDS is the value; an edge's term e = k * r is formed by both of its pixels from
// the same two operands.  So g_u's four edge terms are exactly the e and s that g_gx and g_gy hold.
//
// Barriers.  Every __syncthreads() below is reached by every thread of the block the same number of times: the trip count
// is the kernel argument `rows`, no thread returns early, and lanes past W and rows past H skip the arithmetic and the
// stores, not the barrier.
//
// Memory.  Nothing is indexed at run time but global memory and the two LDS rows (by lane); every view was checked on the
// host against its allocation.  Included by ccp_grid_weighted.hip alone, after ccp_grid_weighted.hpp.
#pragma once

#include "ccp_grid_weighted.hpp"

namespace ccp {

struct ReweightAdjointArgs {
    RobustArgs f;                          // the forward pass as it was described; f.dphi < 0: the plain reweight, no data term
    ImageView grad_wx, grad_wy, grad_lam;  // the upstream gradients, shaped as the weights (absent: +0.0)
    AdjOut g_u, g_gx, g_gy, g_f, g_bwx, g_bwy, g_lam;
};

// psi(q) with d phi / d r_c = psi * r_c, from q and the phi formed of it (`id` is a constant wherever the edge term asks)
__device__ __forceinline__ double reweight_psi(int id, double q, double phi, double eps)
{
    if (id == kPhiCharbonnier) {
        const double p = phi * phi;
        return -(p * phi);
    }
    if (id == kPhiHuber) return sqrt(q) > eps ? -((phi * phi) * phi) : 0.0;      // the kink belongs to the flat side
    if (id == kPhiReciprocal) return q > 0.0 ? -((phi * phi) / sqrt(q)) : 0.0;   // the subgradient at q = 0 is taken as 0
    return 0.0;                                                                  // QUADRATIC
}

// k_x (want & 1), k_y (want & 2) and k_d (want & 4) of pixel (x, y) of set `set`, with the phi each was formed from; +0.0
// for an absent edge or a value not asked for.  The owner asks for all of them, a neighbour for the one k it needs.
template <int PHI>
__device__ __forceinline__ void reweight_adjoint_k(const ReweightAdjointArgs &a, long plane, int x, int y, int set, int want, double &kx,
                                                   double &ky, double &kd, double &px, double &py, double &pd)
{
    const ReweightArgs &r = a.f.r;
    const bool he = x + 1 < r.W, hs = y + 1 < r.H;
    const bool pixel = r.coupling != 0;
    const bool we = he && (want & 1), ws = hs && (want & 2), wl = (want & 4) != 0;
    const bool nx = PHI != kPhiQuadratic && he && (pixel ? (want & 3) != 0 : we);
    const bool ny = PHI != kPhiQuadratic && hs && (pixel ? (want & 3) != 0 : ws);
    const bool nd = wl && a.f.dphi != kPhiQuadratic;
    double qx = 0.0, qy = 0.0, dq = 0.0;
    if (nx || ny || nd) {
        const int c0 = set * r.cpb, c1 = c0 + r.cpb;
        for (int c = c0; c < c1; ++c) {
            const double u = reweight_u(r, plane, x, y, c);
            if (nx) {
                const double d = (r.gx.p ? r.gx.f32(y, x, c) : 0.0) - (reweight_u(r, plane, x + 1, y, c) - u);
                qx += d * d;
            }
            if (ny) {
                const double d = (r.gy.p ? r.gy.f32(y, x, c) : 0.0) - (reweight_u(r, plane, x, y + 1, c) - u);
                qy += d * d;
            }
            if (nd) {
                const double d = a.f.f(y, x, c) - u;
                dq += d * d;
            }
        }
    }
    kx = ky = kd = px = py = pd = 0.0;
    if (pixel) {
        if (we || ws) {                                                    // one phi, one k for both forward edges
            const double q = qx + qy;
            px = py = robust_phi<PHI>(q, r.eps);
            double t = 0.0;
            if (he) {
                const double g = a.grad_wx(y, x, set);
                t += r.bwx.p ? g * r.bwx(y, x, set) : g;
            }
            if (hs) {
                const double g = a.grad_wy(y, x, set);
                t += r.bwy.p ? g * r.bwy(y, x, set) : g;
            }
            kx = ky = (t * r.scale) * reweight_psi(PHI, q, px, r.eps);
        }
    } else {
        if (we) {
            const double g = a.grad_wx(y, x, set);
            px = robust_phi<PHI>(qx, r.eps);
            kx = ((r.bwx.p ? g * r.bwx(y, x, set) : g) * r.scale) * reweight_psi(PHI, qx, px, r.eps);
        }
        if (ws) {
            const double g = a.grad_wy(y, x, set);
            py = robust_phi<PHI>(qy, r.eps);
            ky = ((r.bwy.p ? g * r.bwy(y, x, set) : g) * r.scale) * reweight_psi(PHI, qy, py, r.eps);
        }
    }
    if (wl) {
        const double g = a.grad_lam(y, x, set);
        pd = robust_phi_data(a.f.dphi, dq, a.f.deps);
        kd = ((r.lam.p ? g * r.lam(y, x, set) : g) * a.f.dscale) * reweight_psi(a.f.dphi, dq, pd, a.f.deps);
    }
}

// grid = (ceil(W/kBlock), ceil(H/a.f.rows), sets).  plane: the distance of the handle's x planes (read where a.f.r.u is absent,
// which the entry point refuses: the argument keeps reweight_u's signature).
template <int PHI>
__global__ void __launch_bounds__(kBlock)
k_weighted_reweight_adjoint(ReweightAdjointArgs a, long plane)
{
    __shared__ double east[2][kBlock];
    const ReweightArgs &r = a.f.r;
    const int x = blockIdx.x * kBlock + threadIdx.x, y0 = blockIdx.y * a.f.rows, ch = blockIdx.z;
    const bool column = x < r.W;
    const bool data = a.f.dphi >= 0;
    const int c0 = ch * r.cpb, c1 = c0 + r.cpb;
    const bool he = x + 1 < r.W;
    double kN = 0.0;                                                       // the k_y of the row above
    if (column && y0 >= 1) {
        double t0, t1, t2, t3, t4;
        reweight_adjoint_k<PHI>(a, plane, x, y0 - 1, ch, 2, t0, kN, t1, t2, t3, t4);
    }
    for (int i = 0; i < a.f.rows; ++i) {
        const int y = y0 + i;
        const bool live = column && y < r.H;
        double kx = 0.0, ky = 0.0, kd = 0.0, px = 0.0, py = 0.0, pd = 0.0;
        if (live) reweight_adjoint_k<PHI>(a, plane, x, y, ch, data ? 7 : 3, kx, ky, kd, px, py, pd);
        east[i & 1][threadIdx.x] = kx;
        __syncthreads();                                                   // every thread, every trip
        if (live) {
            double kW = 0.0;
            if (threadIdx.x >= 1) {
                kW = east[i & 1][threadIdx.x - 1];
            } else if (x >= 1) {
                double t0, t1, t2, t3, t4;
                reweight_adjoint_k<PHI>(a, plane, x - 1, y, ch, 1, kW, t0, t1, t2, t3, t4);
            }
            const bool hs = y + 1 < r.H;
            if (a.g_bwx.p) adj_store(a.g_bwx, y, x, ch, he ? a.grad_wx(y, x, ch) * (r.scale * px) : 0.0);
            if (a.g_bwy.p) adj_store(a.g_bwy, y, x, ch, hs ? a.grad_wy(y, x, ch) * (r.scale * py) : 0.0);
            if (a.g_lam.p) adj_store(a.g_lam, y, x, ch, a.grad_lam(y, x, ch) * (a.f.dscale * pd));
            for (int c = c0; c < c1; ++c) {
                const double u = reweight_u(r, plane, x, y, c);
                double t = 0.0, e = 0.0, s = 0.0;
                if (he) {
                    e = kx * ((r.gx.p ? r.gx.f32(y, x, c) : 0.0) - (reweight_u(r, plane, x + 1, y, c) - u));
                    t += e;
                }
                if (hs) {
                    s = ky * ((r.gy.p ? r.gy.f32(y, x, c) : 0.0) - (reweight_u(r, plane, x, y + 1, c) - u));
                    t += s;
                }
                if (x >= 1) t -= kW * ((r.gx.p ? r.gx.f32(y, x - 1, c) : 0.0) - (u - reweight_u(r, plane, x - 1, y, c)));
                if (y >= 1) t -= kN * ((r.gy.p ? r.gy.f32(y - 1, x, c) : 0.0) - (u - reweight_u(r, plane, x, y - 1, c)));
                adj_store(a.g_gx, y, x, c, e);
                adj_store(a.g_gy, y, x, c, s);
                if (data) {
                    const double gf = kd * (a.f.f(y, x, c) - u);
                    adj_store(a.g_f, y, x, c, gf);
                    t -= gf;
                }
                adj_store(a.g_u, y, x, c, t);
            }
            kN = ky;
        }
    }
}

}  // namespace ccp
