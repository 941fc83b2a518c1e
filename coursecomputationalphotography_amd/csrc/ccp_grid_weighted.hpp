// ccp_grid_weighted.hpp — the weighted grid handles (include/ccp_gs.h, CCP_GRID_WEIGHTED), hand-written for gfx950:
// the stored operator's planes and arithmetic, and the operator kernels: the formation with its validation, its
// enqueue-only twins that refresh the values of an installed operator or its values and fixed set, the right-hand side of
// every channel and the coarsening.
//
// Operator.  A weighted handle stores its level-0 operator in four planes of the grid's colour-split layout (w_at,
// the layout of x and b and of the multigrid levels' mg_at): d, we, ws and lambda, pads zero.  we / ws are the weights
// of the edges to the east / south cell (0 where the edge is absent); the weights from the north and west are the
// neighbours' ws / we.  The multigrid V-cycle runs level 0 as a stored operator (kMgCoarse, ccp_grid_mg.hpp) on these
// planes, and its coarsening carries lambda (k_weighted_coarsen, at the end of this file).
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
//
// One operator or one per channel.  The handle keeps `sets` sets of the four planes, 4 x ch_stride doubles apart (d, we,
// ws, lambda of a set one after the other), and, while any set has a fixed pixel or the handle reserves them
// (ccp_grid_reserve_constraints, for ccp_grid_refresh_constrained_device to fill later), `sets` sets of ce, cs, lambda',
// 3 x ch_stride apart: sets = 1 is the operator every channel shares (ccp_grid_set_weights_*), sets = channels gives
// every channel its own (ccp_grid_set_weights_per_channel_device).  A shared operator is a per-channel one with a single
// set that all channels read, and the operator kernels below serve both: the set lies on grid z.  A set without fixed
// pixels beside one that has some carries ce = cs = 0 and lambda' = lambda: w + 0.0 is w for every valid weight but -0.0,
// whose products are zeros that a sum started at +0.0 absorbs, so its right-hand side and hierarchy have the bits of a
// handle without the three extra planes.
//
// This file holds the operator kernels and is included by ccp_grid_weighted.hip alone (a static __global__ function is
// compiled into every translation unit that sees it), which holds every call that launches them; ccp_grid_mg.hip reaches
// the coarsening through a launcher of ccp_grid_weighted_api.hpp.  w_at and weighted_row are in ccp_grid_stencil.hpp.
#pragma once

#include "ccp_grid_adjoint.hpp"        // AdjOut, adj_store: the reweight pass's optional outputs
#include "ccp_grid_mg.hpp"
#include "ccp_view.hpp"

#include <cfloat>

namespace ccp {

__device__ __forceinline__ bool weight_ok(double v) { return v >= 0.0 && v <= DBL_MAX; }   // finite and >= 0 (NaN fails)

// d, we, ws, lambda of every pixel of every set: set k's planes at op + k * op_stride, `plane` doubles apart, from channel
// k of the views wx, wy, lam (H x W for the shared operator).  Every weight is checked by the pixel that owns it (wx(x,y)
// and wy(x,y) by (x,y), where they are read); one failure in any set sets count[0].  grid = (ceil(W/kBlock), H, sets).
static __global__ void __launch_bounds__(kBlock)
k_weighted_coef(ImageView wx, ImageView wy, ImageView lam, int W, int H, long pitch, double *__restrict__ op, long plane, long op_stride,
                unsigned long long *__restrict__ count)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    if (x >= W) return;
    const double l = lam(y, x, ch);
    const double e = x + 1 < W ? wx(y, x, ch) : 0.0;
    const double s = y + 1 < H ? wy(y, x, ch) : 0.0;
    double dd = l;
    if (y >= 1) dd += wy(y - 1, x, ch);
    if (x >= 1) dd += wx(y, x - 1, ch);
    if (x + 1 < W) dd += e;
    if (y + 1 < H) dd += s;
    if (!(weight_ok(l) && weight_ok(e) && weight_ok(s))) atomicOr(count, 1ull);
    double *__restrict__ o = op + (long)ch * op_stride;
    const long at = w_at(pitch, x, y);
    o[at] = dd;
    o[plane + at] = e;
    o[2 * plane + at] = s;
    o[3 * plane + at] = l;
}

// The formation of pixel (x, y) of set `ch` where fixed pixels may exist, ONE body for every kernel below that forms the
// planes described at the top, so that the setter, the refreshes and the reweights cannot drift apart: the check of its
// lambda l and its own east and south weights e, s (+0.0 where the edge is absent), the five fixed flags from
// `fixed_at(x, y)` (a mask view, or the sign of the stored lambda plane), the weights of the edges from the north and the
// west (the neighbours' s and e) from `north()` and `west()` where those edges exist (read from views, formed, or carried
// in a register), the sums dd and lp in their order, the stores and the pixel's three tallies.
// POISON: a lambda that fails the check is stored as +0.0 (every refresh: a refused one poisons the operator's values but
// never its fixed marks, which stay -1); the setter stores it as it is and drops the operator.  CONS: the three extra
// planes exist whatever `cons` says (the mask kernels); otherwise cons is null without them.
// Order.  north() and west() are evaluated after the flags, and the planes' addresses are formed after be / bs, just before
// the first store: the instruction order the kernels had before this function existed, which their pinned register
// counts (tests/test_isa_refresh*.py) depend on.
template <bool POISON, bool CONS, class Fixed, class North, class West>
__device__ __forceinline__ void weighted_form(double l, double e, double s, Fixed fixed_at, North north, West west, int x, int y, int ch, int W,
                                              int H, long pitch, double *op, long plane, long op_stride, double *cons, long cons_stride,
                                              unsigned long long *__restrict__ count, unsigned &n_fixed, unsigned &n_dead, unsigned &n_edges)
{
    if (!(weight_ok(l) && weight_ok(e) && weight_ok(s))) atomicOr(count, 1ull);
    const bool fp = fixed_at(x, y);
    const bool fN = y >= 1 && fixed_at(x, y - 1), fW = x >= 1 && fixed_at(x - 1, y);
    const bool fE = x + 1 < W && fixed_at(x + 1, y), fS = y + 1 < H && fixed_at(x, y + 1);
    const double wN = y >= 1 ? north() : 0.0, wW = x >= 1 ? west() : 0.0;
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
    double *o = op + (long)ch * op_stride;
    const long at = w_at(pitch, x, y);
    o[at] = fp ? 0.0 : dd;
    o[plane + at] = fp || fE ? 0.0 : e;
    o[2 * plane + at] = fp || fS ? 0.0 : s;
    o[3 * plane + at] = fp ? -1.0 : !POISON || weight_ok(l) ? l : 0.0;
    if (CONS || cons) {
        double *k = cons + (long)ch * cons_stride;
        k[at] = be ? e : 0.0;
        k[plane + at] = bs ? s : 0.0;
        k[2 * plane + at] = fp ? 0.0 : lp;
    }
    n_fixed = fp;
    n_dead = !fp && dd == 0.0;
    n_edges = (unsigned)be + (unsigned)bs;
}

// The two kernels that take the fixed set from a mask (channel k of `fixed`, != 0 is fixed), up to their block's counts:
// every set's planes from the four views, every weight checked as k_weighted_coef checks it (the fixed pixels' weights
// too); tally: the block's fixed pixels, free pixels with d = 0 and edges with exactly one fixed end, complete on return.
template <bool POISON>
__device__ __forceinline__ void weighted_mask_block(const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView &fixed, int W,
                                                    int H, long pitch, double *op, long plane, long op_stride, double *cons, long cons_stride,
                                                    unsigned long long *__restrict__ count, unsigned (&tally)[3])
{
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    unsigned n_fixed = 0, n_dead = 0, n_edges = 0;
    if (x < W) {
        const double l = lam(y, x, ch);
        const double e = x + 1 < W ? wx(y, x, ch) : 0.0;
        const double s = y + 1 < H ? wy(y, x, ch) : 0.0;
        weighted_form<POISON, true>(l, e, s, [&](int fx, int fy) { return fixed(fy, fx, ch) != 0; }, [&] { return wy(y - 1, x, ch); },
                                    [&] { return wx(y, x - 1, ch); }, x, y, ch, W, H, pitch, op, plane, op_stride, cons, cons_stride, count,
                                    n_fixed, n_dead, n_edges);
    }
    if (n_fixed) atomicAdd(&tally[0], n_fixed);
    if (n_dead) atomicAdd(&tally[1], n_dead);
    if (n_edges) atomicAdd(&tally[2], n_edges);
    __syncthreads();
}

// k_weighted_coef with a mask of fixed pixels per set: the setter's kernel, ce, cs, lambda' of set k at
// cons + k * cons_stride.  count[0]: the verdict of all sets; count[1 + 3 k ..]: set k's three counts, one atomic per
// non-zero count of a block.  grid = (ceil(W/kBlock), H, sets).
static __global__ void __launch_bounds__(kBlock)
k_weighted_coef_fixed(ImageView wx, ImageView wy, ImageView lam, ImageView fixed, int W, int H, long pitch, double *__restrict__ op, long plane,
                      long op_stride, double *__restrict__ cons, long cons_stride, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally[3];
    weighted_mask_block<false>(wx, wy, lam, fixed, W, H, pitch, op, plane, op_stride, cons, cons_stride, count, tally);
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(count + 1 + 3 * blockIdx.z + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// ccp_grid_refresh_constrained_device: new values AND a new fixed set for the installed operators, on a handle whose
// three extra planes exist: the setter's kernel but for the refresh's poisoned lambda and for where the counts go --
// count[2 + 3 k], count[3 + 3 k] as k_weighted_refresh leaves them, and nfixed[k] set k's fixed pixels, words that only
// this kernel counts into (a value refresh clears count[1 + 3 k] and does not recount it).  Nothing that is read here is
// written here, so there is no in-place question.  grid = (ceil(W/kBlock), H, sets).
static __global__ void __launch_bounds__(kBlock)
k_weighted_fixed_refresh(ImageView wx, ImageView wy, ImageView lam, ImageView fixed, int W, int H, long pitch, double *__restrict__ op,
                         long plane, long op_stride, double *__restrict__ cons, long cons_stride, unsigned long long *__restrict__ count,
                         unsigned long long *__restrict__ nfixed)
{
    __shared__ unsigned tally[3];
    weighted_mask_block<true>(wx, wy, lam, fixed, W, H, pitch, op, plane, op_stride, cons, cons_stride, count, tally);
    const int ch = blockIdx.z;
    if (threadIdx.x == 0 && tally[0]) atomicAdd(nfixed + ch, (unsigned long long)tally[0]);
    if ((threadIdx.x == 1 || threadIdx.x == 2) && tally[threadIdx.x]) atomicAdd(count + 1 + 3 * ch + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// weighted_form for a pass that keeps the fixed set: the flags are the sign of the stored lambda plane (< 0 on a fixed
// pixel), and the fixed pixels are not counted (they do not change).
template <class North, class West>
__device__ __forceinline__ void weighted_refresh_tail(double l, double e, double s, North north, West west, int x, int y, int ch, int W, int H,
                                                      long pitch, double *op, long plane, long op_stride, double *cons, long cons_stride,
                                                      unsigned long long *__restrict__ count, unsigned &n_dead, unsigned &n_edges)
{
    const double *mark = op + (long)ch * op_stride + 3 * plane;
    unsigned n_fixed;
    weighted_form<true, false>(l, e, s, [&](int fx, int fy) { return mark[w_at(pitch, fx, fy)] < 0.0; }, north, west, x, y, ch, W, H, pitch, op,
                               plane, op_stride, cons, cons_stride, count, n_fixed, n_dead, n_edges);
}

// ccp_grid_refresh_weights_device: new values for the installed operators, the fixed set kept.  The planes of every set
// are rewritten as k_weighted_coef_fixed forms them (which, where no pixel is fixed, are k_weighted_coef's: the same
// sums in the same order), the fixed flags from the stored lambda plane (weighted_refresh_tail).  cons: null when the
// handle has no fixed pixel (no plane is negative then, and the three extra planes do not exist).
// The lambda plane is rewritten in place while the neighbours' threads read it.  That is sound because the SIGN of an
// entry never changes here: a fixed pixel's entry is stored as the -1 it holds, a free pixel's as a value that is >= 0 and
// not NaN -- a lambda that fails the check is stored as +0.0, so a refused refresh poisons the operator's values but
// never its fixed marks -- and an aligned 8-byte load returns the old or the new entry, never a mix of the two.
// count[0]: the verdict of all sets, as k_weighted_coef's; count[2 + 3 k], count[3 + 3 k]: set k's free pixels with
// d = 0 and edges with exactly one fixed end (count[1 + 3 k], the fixed pixels, is not touched: they do not change) --
// per block in LDS, then one atomic per non-zero count.  grid = (ceil(W/kBlock), H, sets).
static __global__ void __launch_bounds__(kBlock)
k_weighted_refresh(ImageView wx, ImageView wy, ImageView lam, int W, int H, long pitch, double *op, long plane, long op_stride, double *cons,
                   long cons_stride, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    unsigned n_dead = 0, n_edges = 0;
    if (x < W) {
        const double l = lam(y, x, ch);
        const double e = x + 1 < W ? wx(y, x, ch) : 0.0;
        const double s = y + 1 < H ? wy(y, x, ch) : 0.0;
        weighted_refresh_tail(l, e, s, [&] { return wy(y - 1, x, ch); }, [&] { return wx(y, x - 1, ch); }, x, y, ch, W, H, pitch, op, plane,
                              op_stride, cons, cons_stride, count, n_dead, n_edges);
    }
    if (n_dead) atomicAdd(&tally[0], n_dead);
    if (n_edges) atomicAdd(&tally[1], n_edges);
    __syncthreads();
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(count + 2 + 3 * ch + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// ---- ccp_grid_reweight_device: the weights formed from the solution, never stored ------------------------------------------
// k_weighted_refresh with the reads of wx and wy replaced by arithmetic on u (a view, or the handle's x through w_at) and
// the guidance (include/ccp_gs.h, "Reweighting a weighted operator from the solution", fixes the operation order;
// tests/reweight_helpers.py is the same in numpy).  fp64 throughout, nothing contracted, only +, -, x, / and sqrt: every
// one correctly rounded, so the weights have the model's bits.
//
// One value everywhere.  A thread owns pixel (x, y) and needs four weights: its own e and s, and wN, wW -- the s of
// (x, y-1) and the e of (x-1, y), which those pixels' threads form too.  All of them come from reweight_pixel, the same
// instructions on the same operands in the same order whoever asks, so a weight has one value wherever it is used (and
// only its owner stores it to out_wx / out_wy and has it checked, as k_weighted_refresh's ownership of weight_ok).  With
// CCP_REWEIGHT_PIXEL the neighbour's weight needs the neighbour's other edge: u at (x+1, y-1) and (x-1, y+1) as well.
//
// Memory.  The neighbours' u and guidance are re-read, not staged in LDS: a thread's 3 + 4 extra u reads per channel are
// its lane neighbours' and the adjacent rows' own loads of the same pass and come from L1 / L2 (the rows of a column of
// blocks are scheduled back to back), while a staged halo would cost a barrier and a second addressing path for the
// view / colour-split cases for reads HBM never sees.  NOTES R38.1 has the resource report and the timing.
struct ReweightArgs {
    const double *x;             // the handle's x (colour-split, channels `plane` apart): read where u.p is null
    long pitch;
    int W, H, cpb;               // cpb: channels summed per set (all of them for the shared operator, 1 per channel)
    int coupling;                // CCP_REWEIGHT_EDGE / _PIXEL
    double scale, eps;
    ImageView u, gx, gy, bwx, bwy, lam;
    AdjOut out_wx, out_wy;
};

constexpr int kPhiCharbonnier = 0, kPhiHuber = 1, kPhiReciprocal = 2;      // CCP_REWEIGHT_CHARBONNIER, _HUBER, _RECIPROCAL

template <int PHI>
__device__ __forceinline__ double reweight_phi(double q, double eps)
{
    if (PHI == kPhiCharbonnier) return 1.0 / sqrt(q + eps * eps);
    if (PHI == kPhiHuber) return 1.0 / fmax(sqrt(q), eps);
    return 1.0 / (sqrt(q) + eps);
}

__device__ __forceinline__ double reweight_u(const ReweightArgs &a, long plane, int x, int y, int c)
{
    return a.u.p ? a.u(y, x, c) : a.x[(long)c * plane + w_at(a.pitch, x, y)];
}

// q of the edge from (x, y) to (x + dx, y + dy) (the caller knows it to be inside the canvas) over channels [c0, c1)
// (a view's absence is asked of its pointer here and the default written out, so that no view's `dflt` is live: the pass
// is short of scalar registers, not of anything else)
__device__ __forceinline__ double reweight_q(const ReweightArgs &a, long plane, const ImageView &g, int x, int y, int dx, int dy, int c0, int c1)
{
    double acc = 0.0;
    for (int c = c0; c < c1; ++c) {
        const double r = (g.p ? g.f32(y, x, c) : 0.0) - (reweight_u(a, plane, x + dx, y + dy, c) - reweight_u(a, plane, x, y, c));
        acc += r * r;
    }
    return acc;
}

// The east (want & 1) and south (want & 2) weight of pixel (x, y) of set `set`; +0.0 for an absent edge or one not asked for.
template <int PHI>
__device__ __forceinline__ void reweight_pixel(const ReweightArgs &a, long plane, int x, int y, int set, int want, double &e, double &s)
{
    const bool he = x + 1 < a.W, hs = y + 1 < a.H;
    const int c0 = set * a.cpb, c1 = c0 + a.cpb;
    const bool pixel = a.coupling != 0;
    const double qx = he && (pixel || (want & 1)) ? reweight_q(a, plane, a.gx, x, y, 1, 0, c0, c1) : 0.0;
    const double qy = hs && (pixel || (want & 2)) ? reweight_q(a, plane, a.gy, x, y, 0, 1, c0, c1) : 0.0;
    const double qp = qx + qy;
    e = s = 0.0;
    if (he && (want & 1)) {
        const double t = a.scale * reweight_phi<PHI>(pixel ? qp : qx, a.eps);
        e = a.bwx.p ? a.bwx(y, x, set) * t : t;
    }
    if (hs && (want & 2)) {
        const double t = a.scale * reweight_phi<PHI>(pixel ? qp : qy, a.eps);
        s = a.bwy.p ? a.bwy(y, x, set) * t : t;
    }
}

// op, cons: the sets 4 x plane and 3 x plane apart, as the handle keeps them (cons: null without the three planes); count:
// as k_weighted_refresh's.  grid = (ceil(W/kBlock), H, sets).
template <int PHI>
__global__ void __launch_bounds__(kBlock)
k_weighted_reweight(ReweightArgs a, double *op, long plane, double *cons, unsigned long long *__restrict__ count)
{
    __shared__ unsigned tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, ch = blockIdx.z;
    unsigned n_dead = 0, n_edges = 0;
    if (x < a.W) {
        const double l = a.lam.p ? a.lam(y, x, ch) : 0.0;
        double e, s;
        reweight_pixel<PHI>(a, plane, x, y, ch, 3, e, s);
        adj_store(a.out_wx, y, x, ch, e);
        adj_store(a.out_wy, y, x, ch, s);
        const auto north = [&] {
            double we, ws;
            reweight_pixel<PHI>(a, plane, x, y - 1, ch, 2, we, ws);
            return ws;
        };
        const auto west = [&] {
            double we, ws;
            reweight_pixel<PHI>(a, plane, x - 1, y, ch, 1, we, ws);
            return we;
        };
        weighted_refresh_tail(l, e, s, north, west, x, y, ch, a.W, a.H, a.pitch, op, plane, 4 * plane, cons, 3 * plane, count, n_dead, n_edges);
    }
    if (n_dead) atomicAdd(&tally[0], n_dead);
    if (n_edges) atomicAdd(&tally[1], n_edges);
    __syncthreads();
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(count + 2 + 3 * ch + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// ---- ccp_grid_reweight_robust_device: the edge weights AND lambda formed from the solution ----------------------------------
// k_weighted_reweight with a data term that is reweighted too (include/ccp_gs.h, "Robust data term", fixes the operation
// order; tests/robust_helpers.py is the same in numpy), built so that every weight is formed ONCE: k_weighted_reweight
// forms four weights per pixel of which two are its neighbours', and fp64 sqrt and division bound it (NOTES R38.1).
//
// Geometry.  grid = (ceil(W/kBlock), ceil(H/rows), sets): a thread owns column x and marches down the `rows` rows of its
// strip.  Per row it forms its own e, s and lambda (robust_pixel, one pass over the channels that reads u(x, y) once for
// q_x, q_y and the data residual).  wN is the s it formed for the row above, kept in a register; in the strip's first row
// it forms the s of (x, y0 - 1) itself.  wW is the left lane's e of this row: every lane writes its e to one of two LDS
// rows (east[row & 1]), one barrier, then reads its left neighbour's; lane 0 of a block with x >= 1 forms the e of
// (x - 1, y) itself.  Two rows suffice with one barrier per row: a row's buffer is written again two rows later, and the
// barrier of the row in between lies after every read of it.
//
// Bits.  Whoever forms a weight calls robust_pixel -- the same instructions on the same operands in the same order, every
// one of them a correctly rounded fp64 operation -- and a value that went through a register or LDS is the value, so a
// weight has one value wherever it is used, as in k_weighted_reweight.  With CCP_REWEIGHT_PIXEL the two forward edges of
// a pixel share one phi; with _EDGE each has its own; lambda costs one more unless its penalty is QUADRATIC.
//
// Barriers.  Every __syncthreads() below is reached by every thread of the block the same number of times: the trip count
// is the kernel argument `rows`, no thread returns early, and lanes past W and rows past H skip the arithmetic and the
// stores, not the barrier.
//
// The tail is weighted_refresh_tail, with callables that hand over the two carried weights; the thread's tallies are
// summed over its rows before the block's one atomic per non-zero count.
constexpr int kPhiQuadratic = 3;                                          // CCP_REWEIGHT_QUADRATIC: phi = 1.0, q not formed

struct RobustArgs {
    ReweightArgs r;              // the edge term, as k_weighted_reweight's; r.lam: the base lambda (null: 1)
    int rows;                    // rows per strip: every thread makes exactly this many trips
    int dphi;                    // the data penalty, CCP_REWEIGHT_* (uniform over the launch)
    double dscale, deps;
    ImageView f;                 // null only with dphi == kPhiQuadratic
    AdjOut out_lam;
};

template <int PHI>
__device__ __forceinline__ double robust_phi(double q, double eps)
{
    if constexpr (PHI == kPhiQuadratic)
        return 1.0;
    else
        return reweight_phi<PHI>(q, eps);
}

__device__ __forceinline__ double robust_phi_data(int phi, double q, double eps)
{
    if (phi == kPhiCharbonnier) return reweight_phi<kPhiCharbonnier>(q, eps);
    if (phi == kPhiHuber) return reweight_phi<kPhiHuber>(q, eps);
    if (phi == kPhiReciprocal) return reweight_phi<kPhiReciprocal>(q, eps);
    return 1.0;
}

// The east (want & 1) and south (want & 2) weight and the lambda (want & 4) of pixel (x, y) of set `set`; +0.0 for an
// absent edge or a value not asked for.  The owner asks for all three, a neighbour for the one weight it needs.
template <int PHI>
__device__ __forceinline__ void robust_pixel(const RobustArgs &a, long plane, int x, int y, int set, int want, double &e, double &s, double &l)
{
    const ReweightArgs &r = a.r;
    const bool he = x + 1 < r.W, hs = y + 1 < r.H;
    const bool pixel = r.coupling != 0;
    const bool we = he && (want & 1), ws = hs && (want & 2), wl = (want & 4) != 0;
    // which sums are formed: with PIXEL coupling either weight needs both of the pixel's edges
    const bool nx = PHI != kPhiQuadratic && he && (pixel ? (want & 3) != 0 : we);
    const bool ny = PHI != kPhiQuadratic && hs && (pixel ? (want & 3) != 0 : ws);
    const bool nd = wl && a.dphi != kPhiQuadratic;
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
                const double d = a.f(y, x, c) - u;
                dq += d * d;
            }
        }
    }
    double te = 0.0, ts = 0.0;
    if (pixel) {
        if (we || ws) te = ts = r.scale * robust_phi<PHI>(qx + qy, r.eps);     // one phi for both forward edges
    } else {
        if (we) te = r.scale * robust_phi<PHI>(qx, r.eps);
        if (ws) ts = r.scale * robust_phi<PHI>(qy, r.eps);
    }
    e = s = l = 0.0;
    if (we) e = r.bwx.p ? r.bwx(y, x, set) * te : te;
    if (ws) s = r.bwy.p ? r.bwy(y, x, set) * ts : ts;
    if (wl) {
        const double t = a.dscale * robust_phi_data(a.dphi, dq, a.deps);
        l = r.lam.p ? r.lam(y, x, set) * t : t;
    }
}

// op, cons, count: as k_weighted_reweight's.  grid = (ceil(W/kBlock), ceil(H/a.rows), sets).
template <int PHI>
__global__ void __launch_bounds__(kBlock)
k_weighted_reweight_robust(RobustArgs a, double *op, long plane, double *cons, unsigned long long *__restrict__ count)
{
    __shared__ double east[2][kBlock];
    __shared__ unsigned tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y0 = blockIdx.y * a.rows, ch = blockIdx.z;
    const bool column = x < a.r.W;
    unsigned t_dead = 0, t_edges = 0;
    double wN = 0.0;                                                       // the s of the row above
    if (column && y0 >= 1) {
        double ne, nl;
        robust_pixel<PHI>(a, plane, x, y0 - 1, ch, 2, ne, wN, nl);
    }
    for (int i = 0; i < a.rows; ++i) {
        const int y = y0 + i;
        const bool live = column && y < a.r.H;
        double e = 0.0, s = 0.0, l = 0.0;
        if (live) robust_pixel<PHI>(a, plane, x, y, ch, 7, e, s, l);
        east[i & 1][threadIdx.x] = e;
        __syncthreads();                                                   // every thread, every trip
        if (live) {
            double wW = 0.0;
            if (threadIdx.x >= 1) {
                wW = east[i & 1][threadIdx.x - 1];
            } else if (x >= 1) {
                double ws, wl;
                robust_pixel<PHI>(a, plane, x - 1, y, ch, 1, wW, ws, wl);
            }
            adj_store(a.r.out_wx, y, x, ch, e);
            adj_store(a.r.out_wy, y, x, ch, s);
            adj_store(a.out_lam, y, x, ch, l);
            unsigned n_dead = 0, n_edges = 0;
            weighted_refresh_tail(l, e, s, [&] { return wN; }, [&] { return wW; }, x, y, ch, a.r.W, a.r.H, a.r.pitch, op, plane, 4 * plane, cons,
                                  3 * plane, count, n_dead, n_edges);
            t_dead += n_dead;
            t_edges += n_edges;
            wN = s;
        }
    }
    if (t_dead) atomicAdd(&tally[0], t_dead);
    if (t_edges) atomicAdd(&tally[1], t_edges);
    __syncthreads();
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(count + 2 + 3 * ch + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// b of `cpb` channels per block from one set of the stored operator: block z takes channels [z cpb, (z + 1) cpb) and the
// set at op + z * op_stride (d, we, ws, lambda planes `plane` doubles apart) and cons + z * cons_stride (ce, cs).  The
// shared operator runs as grid z = 1, cpb = C: the weights are read once per pixel and the channels looped.  One
// operator per channel runs as grid z = C, cpb = 1.  gx, gy (f32: read as such), f, v (u8, f32 or f64) are H x W x C; has & 1: gx,
// & 2: gy, & 4: f, & 8: v, a missing one reads 0.  INIT: x := f on live pixels, 0 on dead ones.
// FIXED: some set has fixed pixels (cons is there; the lambda plane < 0 marks them): the guidance terms take the
// original weights we + ce, ws + cs, the prescribed values v of the fixed neighbours enter b, and a fixed pixel gets
// b = 0, x := v.  grid = (ceil(W/kBlock), H, sets).
template <bool INIT, bool FIXED>
__global__ void __launch_bounds__(kBlock)
k_weighted_rhs(double *__restrict__ b, double *__restrict__ xo, Geom g, const double *__restrict__ op, long plane, long op_stride,
               const double *__restrict__ cons, long cons_stride, ImageView gx, ImageView gy, ImageView f, ImageView v, int has, int cpb)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, set = blockIdx.z;
    if (x >= g.W) return;
    const double *__restrict__ d = op + (long)set * op_stride, *__restrict__ we = d + plane, *__restrict__ ws = d + 2 * plane,
                 *__restrict__ lam = d + 3 * plane;
    const int c0 = set * cpb, c1 = c0 + cpb;
    const long at = w_at(g.pitch, x, y);
    double wN = y >= 1 ? ws[w_at(g.pitch, x, y - 1)] : 0.0, wW = x >= 1 ? we[w_at(g.pitch, x - 1, y)] : 0.0;
    double wE = we[at], wS = ws[at];
    const double l = lam[at];
    const bool live = d[at] != 0.0;
    const bool hx = has & 1, hy = has & 2, hf = has & 4, hv = has & 8;
    bool fN = false, fW = false, fE = false, fS = false;
    if (FIXED) {
        const double *__restrict__ ce = cons + (long)set * cons_stride, *__restrict__ cs = ce + plane;
        if (l < 0.0) {                                                      // a fixed pixel
            for (int c = c0; c < c1; ++c) {
                b[(long)c * g.ch_stride + at] = 0.0;
                xo[(long)c * g.ch_stride + at] = hv ? v(y, x, c) : 0.0;
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
    for (int c = c0; c < c1; ++c) {
        const double fv = hf ? f(y, x, c) : 0.0;
        double t = 0.0;
        if (y >= 1) t += wN * (hy ? gy.f32(y - 1, x, c) : 0.0);
        if (x >= 1) t += wW * (hx ? gx.f32(y, x - 1, c) : 0.0);
        if (x + 1 < g.W) t += -(wE * (hx ? gx.f32(y, x, c) : 0.0));
        if (y + 1 < g.H) t += -(wS * (hy ? gy.f32(y, x, c) : 0.0));
        t += l * fv;
        if (FIXED) {
            if (fN) t += wN * (hv ? v(y - 1, x, c) : 0.0);
            if (fW) t += wW * (hv ? v(y, x - 1, c) : 0.0);
            if (fE) t += wE * (hv ? v(y, x + 1, c) : 0.0);
            if (fS) t += wS * (hv ? v(y + 1, x, c) : 0.0);
        }
        b[(long)c * g.ch_stride + at] = t;
        if (INIT) xo[(long)c * g.ch_stride + at] = live ? fv : 0.0;
    }
}

// Level k+1 of `sets` hierarchies (one: the shared operator's; one per channel otherwise) from their levels k, the set on
// grid z: set ch's fine d, we, ws are lv's pointers + ch * fs, its lambda lam + ch * ls; its coarse planes d, we, ws,
// lam_c + ch * cstride.  grid = (ceil(Wc/kBlock), Hc, sets).
static __global__ void __launch_bounds__(kBlock)
k_weighted_coarsen(MgLevel lv, long fs, const double *__restrict__ lam, long ls, MgLevel cv, double *__restrict__ d, double *__restrict__ we,
                   double *__restrict__ ws, double *__restrict__ lam_c, long cstride, double edge)
{
    const int X = blockIdx.x * kBlock + threadIdx.x, Y = blockIdx.y;
    if (X >= cv.W) return;
    const long ch = blockIdx.z;
    lv.d += ch * fs;
    lv.we += ch * fs;
    lv.ws += ch * fs;
    const long co = ch * cstride;
    mg_coarsen_weighted_cell(lv, lam + ch * ls, cv, X, Y, d + co, we + co, ws + co, lam_c + co, edge);
}

// ---- weighted handles (ccp_grid_weighted.hpp explains the operator's planes) ----------------------------------------------

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
