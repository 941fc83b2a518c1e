// ccp_grid_weighted.hip — everything only a weighted handle (CCP_GRID_WEIGHTED) accepts: its operator, right-hand side,
// constraint counts, product and adjoints, with the operator kernels (ccp_grid_weighted.hpp, ccp_grid_adjoint.hpp,
// ccp_grid_reweight_adjoint.hpp, ccp_grid_irls_adjoint.hpp); and the
// launchers of the coarsening and of the per-channel batched mode's kernels (ccp_grid_pco.hpp) that ccp_grid_mg.hip calls
// (ccp_grid_weighted_api.hpp).
#include "ccp_grid_handle.hpp"
#include "ccp_grid_pco.hpp"
#include "ccp_grid_weighted.hpp"
#include "ccp_grid_reweight_adjoint.hpp"
#include "ccp_grid_irls_adjoint.hpp"
#include "ccp_grid_adjoint.hpp"
#include "ccp_grid_weighted_api.hpp"
#include "ccp_view_check.hpp"

#include <atomic>

using namespace ccp;

namespace {

dim3 pixels(int W, int H, int C) { return dim3((unsigned)((W + kBlock - 1) / kBlock), (unsigned)H, (unsigned)C); }

// The planes of `sets` operators (1: the one all channels share, from H x W views; C: one per channel) in one launch;
// fixed: null for none (cons is not touched then).  count: 1 + 3 sets words, zeroed here.
int weighted_coef(hipStream_t s, const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView *fixed, int W, int H,
                  int sets, long pitch, double *op, long plane, double *cons, unsigned long long *count)
{
    CCP_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long) * (size_t)(1 + 3 * sets), s));
    if (fixed)
        hipLaunchKernelGGL(k_weighted_coef_fixed, pixels(W, H, sets), dim3(kBlock), 0, s, wx, wy, lam, *fixed, W, H, pitch, op, plane, 4 * plane,
                           cons, 3 * plane, count);
    else
        hipLaunchKernelGGL(k_weighted_coef, pixels(W, H, sets), dim3(kBlock), 0, s, wx, wy, lam, W, H, pitch, op, plane, 4 * plane, count);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// b (and x at fixed pixels, or everywhere with init) of all C channels from `sets` operators in one launch; cons: null
// without fixed pixels
int weighted_rhs(hipStream_t s, double *b, double *x, const Geom &g, int C, int sets, const double *op, const double *cons,
                 const ImageView &gx, const ImageView &gy, const ImageView &f, const ImageView &v, int has, bool init)
{
    const long plane = g.ch_stride;
    const dim3 grid = pixels(g.W, g.H, sets);
    with_bool(init, [&](auto I) {
        with_bool(cons != nullptr, [&](auto F) {
            hipLaunchKernelGGL((k_weighted_rhs<decltype(I)::value, decltype(F)::value>), grid, dim3(kBlock), 0, s, b, x, g, op, plane, 4 * plane,
                               cons, 3 * plane, gx, gy, f, v, cons ? has : has & 7, C / sets);
        });
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

}  // namespace

int ccp::weighted_coarsen(hipStream_t s, int sets, const MgLevel &lv, long fs, const double *lam, long ls, const MgLevel &cv, double *d,
                          double *we, double *ws, double *lam_c, long cstride, double edge)
{
    hipLaunchKernelGGL(k_weighted_coarsen, pixels(cv.W, cv.H, sets), dim3(kBlock), 0, s, lv, fs, lam, ls, cv, d, we, ws, lam_c, cstride, edge);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// k_pco_tile's five planes pass the 64 KiB a kernel may take without asking (115,200 B at nu = 2): once per device and process
int ccp::pco_tile_lds_limit()
{
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    CCP_HIP(hipGetDevice(&dev));
    const unsigned long long bit = dev < 64 ? 1ull << dev : 0;
    if (raised.load() & bit) return CCP_OK;
    const int bytes = mgb_tile_lds(kMgCoarse, 4);                    // the largest nu
    CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pco_tile<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pco_tile<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    raised.fetch_or(bit);
    return CCP_OK;
}

int ccp::pco_tile(hipStream_t s, bool post, dim3 tiles, int C, const MgLevel &lv, long os, const double *b, const double *z_in, double *z_out,
                  long fs, const MgLevel &cv, const double *ec, long es, double cs, int nu, const CgState *st)
{
    tiles.z = (unsigned)C;
    with_bool(post, [&](auto P) {
        hipLaunchKernelGGL((k_pco_tile<decltype(P)::value>), tiles, dim3(mgb_tile_threads(kMgCoarse)), mgb_tile_lds(kMgCoarse, nu), s, lv, os, b,
                           z_in, z_out, fs, cv, ec, es, cs, nu, st);
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_restrict(hipStream_t s, int C, const MgLevel &lv, long os, const double *b, const double *z, long fs, const MgLevel &cv, double *bc,
                      long es, const CgState *st)
{
    hipLaunchKernelGGL(k_pco_restrict, pixels(cv.W, cv.H, C), dim3(kBlock), 0, s, lv, os, b, z, fs, cv, bc, es, st);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_tail(hipStream_t s, int C, const MgTail *tails, const double *b_top, double *z_top, long bs, long zs, double cs, int nu,
                  const CgState *st)
{
    hipLaunchKernelGGL(k_pco_tail, dim3((unsigned)C), dim3(kBlock), 0, s, tails, b_top, z_top, bs, zs, cs, nu, st);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_apply(hipStream_t s, bool dot, dim3 grid, int C, const MgLevel &lv, long os, const double *in, double *out, long vs,
                   double *partial, long ps, const CgState *st)
{
    grid.z = 2 * (unsigned)C;
    with_bool(dot, [&](auto D) {
        hipLaunchKernelGGL((k_pco_apply<decltype(D)::value>), grid, dim3(kBlock), 0, s, lv, os, in, out, vs, partial, ps, st);
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// ============================================================================================
// Weighted grids (include/ccp_gs.h, CCP_GRID_WEIGHTED; kernels: ccp_grid_weighted.hpp)
// ============================================================================================
namespace {

// every entry point here begins with this: bind, then CCP_ERR_UNSUPPORTED on a handle that is not weighted
int weighted_handle(ccp_grid *g)
{
    CCP_TRY(bind(g));
    return g->weighted ? CCP_OK : CCP_ERR_UNSUPPORTED;
}

// b of every channel from the handle's operator, the shared one or every channel's own, in one launch; v: gx, gy, f and
// the prescribed values (has & 1, 2, 4, 8: which of them are there)
int weighted_rhs_launch(ccp_grid *g, const ImageView v[4], int has, bool init_x)
{
    const int C = g->desc.channels;
    return weighted_rhs(g->stream, g->b.p, g->x.p, g->geom, C, g->per_channel ? C : 1, g->wop.p, g->has_fixed ? g->wcons.p : nullptr, v[0], v[1],
                        v[2], v[3], has, init_x);
}

// ccp_grid_assemble_weighted_rhs and ccp_grid_assemble_constrained_rhs: the host arrays staged, one launch, one wait
int weighted_rhs_host(ccp_grid *g, const float *gx, const float *gy, int64_t field_stride_bytes, const float *f, int64_t f_stride_bytes,
                      const float *values, int64_t values_stride_bytes, bool init_x)
{
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    const int64_t row = (int64_t)W * C * (int64_t)sizeof(float);
    if ((gx || gy) && field_stride_bytes < row) return CCP_ERR_BAD_ARG;
    if (f && f_stride_bytes < row) return CCP_ERR_BAD_ARG;
    if (values && values_stride_bytes < row) return CCP_ERR_BAD_ARG;
    if (!g->has_op) return CCP_ERR_STATE;
    const float *src[4] = {gx, gy, f, values};
    const int64_t stride[4] = {field_stride_bytes, field_stride_bytes, f_stride_bytes, values_stride_bytes};
    DevBuf<float> dev[4];
    ImageView v[4];
    int has = 0;
    for (int i = 0; i < 4; ++i) {
        v[i] = ImageView{nullptr, 0, 0, 0, 0, 0.0};
        if (!src[i]) continue;
        has |= 1 << i;
        CCP_TRY(upload_window(g, dev[i], src[i], stride[i], 0, H));
        v[i] = ImageView{dev[i].p, (long)W * C, (long)C, 1, CCP_DTYPE_F32, 0.0};   // the staging buffer: packed H x W x C
    }
    CCP_TRY(weighted_rhs_launch(g, v, has, init_x));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
}

int weighted_rhs_device(ccp_grid *g, const ccp_device_array *gx, const ccp_device_array *gy, const ccp_device_array *f,
                        const ccp_device_array *values, bool init)
{
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    if (gx) CCP_TRY(check_view(g, gx, kF32, false, 1, H, W, C));
    if (gy) CCP_TRY(check_view(g, gy, kF32, false, 1, H, W, C));
    if (f) CCP_TRY(check_view(g, f, kF32F64 | kU8, false, 1, H, W, C));
    if (values) CCP_TRY(check_view(g, values, kF32F64 | kU8, false, 1, H, W, C));
    if (!g->has_op) return CCP_ERR_STATE;
    const int has = (gx ? 1 : 0) | (gy ? 2 : 0) | (f ? 4 : 0) | (values ? 8 : 0);
    const ImageView v[4] = {image_view(gx, 0.0), image_view(gy, 0.0), image_view(f, 0.0), image_view(values, 0.0)};
    return weighted_rhs_launch(g, v, has, init);
}

// a new operator is coming: the old one, its counts and the hierarchy built on it go
void drop_operator(ccp_grid *g)
{
    mg_release(&g->mg);
    g->has_op = g->has_fixed = false;
    g->per_channel = false;
    g->refreshed = false;
    g->fixed_on_device = false;
    g->mg_nullspace.forget();
}

// ccp_grid_constraint_info after a refresh: the counts the refresh pass left on the device (one wait).  Read at every call
// and not once per refresh: a refresh that a captured graph replays changes them without the host taking part.
int refreshed_counts(ccp_grid *g)
{
    const int sets = g->per_channel ? g->desc.channels : 1;
    unsigned long long count[kRefreshCounts] = {};
    // (after a constrained refresh the fixed pixels are the device's too: the words behind the others, in the same copy)
    const int words = g->fixed_on_device ? kRefreshFixedAt + sets : 1 + 3 * sets;
    CCP_HIP(hipMemcpyAsync(count, g->rcount.p, sizeof(unsigned long long) * (size_t)words, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    for (int c = 0; c < sets; ++c) {
        if (g->fixed_on_device) g->pc_fixed[c] = (long)count[kRefreshFixedAt + c];
        g->pc_live[c] = (long)g->geom.W * g->geom.H - g->pc_fixed[c] - (long)count[2 + 3 * c];
        g->pc_edges[c] = (long)count[3 + 3 * c];
    }
    return CCP_OK;
}

// wop for `sets` operators (1: the shared one; channels: one per channel), pads zero; what it held is gone
int operator_planes(ccp_grid *g, int sets)
{
    if (g->op_sets == sets) return CCP_OK;
    const size_t count = 4 * (size_t)sets * (size_t)g->geom.ch_stride;
    g->op_sets = 0;
    CCP_TRY(g->wop.alloc(count));
    CCP_HIP(hipMemsetAsync(g->wop.p, 0, sizeof(double) * count, g->stream));
    g->op_sets = sets;
    return CCP_OK;
}

// The handle's operators (one that all channels share, the views H x W; or per_channel: one per channel, the views
// H x W x C) from three weight views and, with `fixed`, a mask of fixed pixels: all planes in one launch, the verdict
// and, with a mask, every set's counts in one read.  The old operator and the hierarchy built on it are gone either
// way: a refusal leaves the handle with none.  The three extra planes stay only if some set has a fixed pixel or the
// handle reserves them (ccp_grid_reserve_constraints; no mask is the all-zero mask then): with no fixed pixel the four
// planes are what the call without a mask forms, bit for bit.
int form_operator(ccp_grid *g, bool per_channel, const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView *fixed)
{
    const Geom &geo = g->geom;
    const long n = geo.ch_stride;
    const int sets = per_channel ? g->desc.channels : 1;
    // a setter's operator is validated on the host: the status word of an earlier refresh goes, since the enqueue solve
    // reads the word whoever installed the operator (a handle that was never refreshed launches what it launched)
    if (g->refreshed) CCP_HIP(hipMemsetAsync(g->op_status.p, 0, sizeof(unsigned), g->stream));
    drop_operator(g);
    g->wcons.release();
    CCP_TRY(operator_planes(g, sets));
    const ImageView none{nullptr, 0, 0, 0, CCP_DTYPE_U8, 0.0};
    if (!fixed && g->reserve_cons) fixed = &none;
    if (fixed) {
        CCP_TRY(g->wcons.alloc(3 * (size_t)sets * (size_t)n));
        CCP_HIP(hipMemsetAsync(g->wcons.p, 0, 3 * sizeof(double) * (size_t)sets * (size_t)n, g->stream));   // the pads
    }
    CCP_TRY(weighted_coef(g->stream, wx, wy, lam, fixed, geo.W, geo.H, sets, geo.pitch, g->wop.p, n, g->wcons.p, g->wcount.p));
    unsigned long long count[1 + 3 * kMaxChannels] = {1};
    CCP_HIP(hipMemcpyAsync(count, g->wcount.p, sizeof(unsigned long long) * (size_t)(1 + 3 * sets), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    bool any_fixed = false;
    for (int c = 0; c < sets && fixed; ++c) any_fixed = any_fixed || count[1 + 3 * c] != 0;
    const bool keep = !count[0] && (any_fixed || g->reserve_cons);
    if (!keep) g->wcons.release();
    if (count[0]) return CCP_ERR_BAD_ARG;
    for (int c = 0; c < sets; ++c) {
        g->pc_fixed[c] = fixed ? (long)count[1 + 3 * c] : 0;
        g->pc_live[c] = fixed ? (long)geo.W * geo.H - (long)count[1 + 3 * c] - (long)count[2 + 3 * c] : -1;
        g->pc_edges[c] = fixed ? (long)count[3 + 3 * c] : 0;
    }
    g->has_op = true;
    g->per_channel = per_channel;
    g->has_fixed = keep;                                                   // the three planes exist
    return edge_timeout_status(g);
}

// a channel's dead pixels counted once (an operator formed without a mask)
int count_live(ccp_grid *g, const double *d, long *live)
{
    const Geom &geo = g->geom;
    unsigned long long dead = 0;
    CCP_HIP(hipMemsetAsync(g->wcount.p, 0, sizeof(unsigned long long), g->stream));
    hipLaunchKernelGGL(k_weighted_count_dead, pixel_grid(g, geo.H), dim3(kBlock), 0, g->stream, d, geo.W, geo.H, geo.pitch, g->wcount.p);
    CCP_HIP(hipGetLastError());
    CCP_HIP(hipMemcpyAsync(&dead, g->wcount.p, sizeof(dead), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    *live = (long)geo.W * geo.H - (long)dead;
    return CCP_OK;
}

// the three weight views of a setter or a refresh, checked in their order (H x W x channels); an absent one reads 1, 1, 0
int weight_views(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda, int channels,
                 ImageView v[3])
{
    const ccp_device_array *src[3] = {wx, wy, lambda};
    const double dflt[3] = {1.0, 1.0, 0.0};
    for (int i = 0; i < 3; ++i) {
        if (src[i]) CCP_TRY(check_view(g, src[i], kF32F64, false, 1, g->geom.H, g->geom.W, channels));
        v[i] = image_view(src[i], dflt[i]);
    }
    return CCP_OK;
}

// ccp_grid_set_weights_[constrained_]device and ccp_grid_set_weights_per_channel_device: the views are H x W for the
// shared operator and H x W x channels for one operator per channel
int set_weights_device(ccp_grid *g, bool per_channel, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                       const ccp_device_array *fixed)
{
    CCP_TRY(weighted_handle(g));
    const int C = per_channel ? g->desc.channels : 1;
    ImageView v[3];
    CCP_TRY(weight_views(g, wx, wy, lambda, C, v));
    if (!fixed) return form_operator(g, per_channel, v[0], v[1], v[2], nullptr);
    CCP_TRY(check_view(g, fixed, kF32F64 | kU8, false, 1, g->geom.H, g->geom.W, C));
    const ImageView m = image_view(fixed, 0.0);
    return form_operator(g, per_channel, v[0], v[1], v[2], &m);
}

// b := A x (MODE 0) or the residual's partial sums (MODE 1) of every channel of a weighted handle.  With one operator
// per channel the same kernel runs once per channel on that channel's planes, vectors and slice of the partial sums:
// the launch a one-channel handle makes.
template <int MODE>
int weighted_apply_mode(ccp_grid *g)
{
    dim3 grid = weighted_apply_grid(g);
    const long n = g->geom.ch_stride;
    if (!g->per_channel) {
        hipLaunchKernelGGL((k_weighted_apply<MODE>), grid, dim3(kBlock), 0, g->stream, g->x.p, g->b.p, g->geom, g->wop.p, n, g->wpart.p);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    grid.z = 2;
    for (int ch = 0; ch < g->desc.channels; ++ch) {
        hipLaunchKernelGGL((k_weighted_apply<MODE>), grid, dim3(kBlock), 0, g->stream, g->x.p + ch * n, g->b.p + ch * n, g->geom,
                           g->wop.p + 4 * ch * n, n, g->wpart.p + 4L * ch * grid.x);
        CCP_HIP(hipGetLastError());
    }
    return CCP_OK;
}

// Every enqueue-only pass that gives the installed operators new values: `launch` enqueues the kernel that rewrites level 0
// and counts into the first `words` words of rcount, which mg_refresh_begin clears with the status word; mg_refresh rebuilds
// what mg_prepare derived.  Launches on the handle's stream, nothing else.
template <typename Launch>
int refresh_pass(ccp_grid *g, int words, Launch &&launch)
{
    CCP_TRY(mg_refresh_begin(g, words));
    launch();
    CCP_HIP(hipGetLastError());
    g->refreshed = true;
    g->mg_nullspace.floating = -1;      // the census verdict the host remembers is the old values': a later prepare or solve asks again
    return mg_refresh(g);
}

// ccp_grid_refresh_weights_device (with_mask false: the fixed set the lambda plane marks is kept) and
// ccp_grid_refresh_constrained_device (the fixed set of `fixed`, NULL: the empty one)
int refresh_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                   const ccp_device_array *fixed, bool with_mask)
{
    CCP_TRY(weighted_handle(g));
    if (!g->has_op) return CCP_ERR_STATE;                                  // (the operator's kind decides the views' extents)
    const Geom &geo = g->geom;
    const int sets = g->per_channel ? g->desc.channels : 1;
    ImageView v[3];
    CCP_TRY(weight_views(g, wx, wy, lambda, sets, v));
    if (fixed) CCP_TRY(check_view(g, fixed, kF32F64 | kU8, false, 1, geo.H, geo.W, sets));
    if (with_mask && !g->has_fixed) return CCP_ERR_STATE;                  // the three planes: reserved, or a setter's mask had a fixed pixel
    const long n = geo.ch_stride;
    if (!with_mask)
        return refresh_pass(g, 1 + 3 * sets, [&] {
            hipLaunchKernelGGL(k_weighted_refresh, pixels(geo.W, geo.H, sets), dim3(kBlock), 0, g->stream, v[0], v[1], v[2], geo.W, geo.H,
                               geo.pitch, g->wop.p, n, 4 * n, g->has_fixed ? g->wcons.p : nullptr, 3 * n, g->rcount.p);
        });
    // a new fixed set: its words behind the others are cleared and counted too, and ccp_grid_constraint_info reads them from now on
    return refresh_pass(g, kRefreshFixedAt + sets, [&] {
        hipLaunchKernelGGL(k_weighted_fixed_refresh, pixels(geo.W, geo.H, sets), dim3(kBlock), 0, g->stream, v[0], v[1], v[2],
                           image_view(fixed, 0.0), geo.W, geo.H, geo.pitch, g->wop.p, n, 4 * n, g->wcons.p, 3 * n, g->rcount.p,
                           g->rcount.p + kRefreshFixedAt);
        g->fixed_on_device = true;
    });
}

AdjOut adj_out(const ccp_device_array *a);                               // (with the adjoint pass, below)

static_assert(kPhiCharbonnier == CCP_REWEIGHT_CHARBONNIER && kPhiHuber == CCP_REWEIGHT_HUBER && kPhiReciprocal == CCP_REWEIGHT_RECIPROCAL,
              "k_weighted_reweight's PHI is the header's penalty id");
static_assert(kPhiQuadratic == CCP_REWEIGHT_QUADRATIC, "k_weighted_reweight_robust's PHI is the header's penalty id");

// a checked penalty id as a template argument: f(P) with decltype(P)::value == penalty (as with_bool, for the kernels' PHI)
template <typename F>
void with_phi(int penalty, F &&f)
{
    if (penalty == kPhiCharbonnier) f(std::integral_constant<int, kPhiCharbonnier>{});
    else if (penalty == kPhiHuber) f(std::integral_constant<int, kPhiHuber>{});
    else if (penalty == kPhiReciprocal) f(std::integral_constant<int, kPhiReciprocal>{});
    else f(std::integral_constant<int, kPhiQuadratic>{});
}

// the bytes [lo, hi) a view of extents H x W x C spans
void view_span(const ccp_device_array *a, long H, long W, long C, uintptr_t *lo, uintptr_t *hi)
{
    const unsigned long long last = (unsigned long long)(H - 1) * (unsigned long long)a->stride_y +
                                    (unsigned long long)(W - 1) * (unsigned long long)a->stride_x +
                                    (unsigned long long)(C - 1) * (unsigned long long)a->stride_c;
    *lo = (uintptr_t)a->data;
    *hi = *lo + (uintptr_t)((last + 1) * dtype_bytes(a->dtype));
}

bool reweight_numbers_ok(double scale, double epsilon, bool with_epsilon)
{
    return (!with_epsilon || (epsilon > 0.0 && epsilon <= DBL_MAX)) && scale >= 0.0 && scale <= DBL_MAX;
}

// What ccp_grid_reweight_device (data: null) and ccp_grid_reweight_robust_device check on the host before anything is
// enqueued, in one place, and the kernels' description of the edge term: the numbers, the installed operator, every view,
// and that no output shares bytes with an input.
int reweight_checked(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data, ReweightArgs *a)
{
    CCP_TRY(weighted_handle(g));
    if (!how) return CCP_ERR_BAD_ARG;
    const int last_penalty = data ? CCP_REWEIGHT_QUADRATIC : CCP_REWEIGHT_RECIPROCAL;
    if (how->penalty < CCP_REWEIGHT_CHARBONNIER || how->penalty > last_penalty) return CCP_ERR_BAD_ARG;
    if (how->coupling != CCP_REWEIGHT_EDGE && how->coupling != CCP_REWEIGHT_PIXEL) return CCP_ERR_BAD_ARG;
    if (!reweight_numbers_ok(how->scale, how->epsilon, true)) return CCP_ERR_BAD_ARG;
    if (data) {
        if (data->penalty < CCP_REWEIGHT_CHARBONNIER || data->penalty > CCP_REWEIGHT_QUADRATIC || data->reserved != 0) return CCP_ERR_BAD_ARG;
        if (!reweight_numbers_ok(data->scale, data->epsilon, data->penalty != CCP_REWEIGHT_QUADRATIC)) return CCP_ERR_BAD_ARG;
        if (!data->f && data->penalty != CCP_REWEIGHT_QUADRATIC) return CCP_ERR_BAD_ARG;
    }
    if (!g->has_op) return CCP_ERR_STATE;                                  // (the operator's kind decides the views' extents)
    const Geom &geo = g->geom;
    const int C = g->desc.channels, sets = g->per_channel ? C : 1;
    constexpr int kInputs = 7, kViews = 10;
    struct {
        const ccp_device_array *a;
        unsigned dtypes;
        bool output;
        int c;
    } views[kViews] = {{how->u, kF32F64 | kU8, false, C},
                       {how->gx, kF32, false, C},
                       {how->gy, kF32, false, C},
                       {how->base_wx, kF32F64, false, sets},
                       {how->base_wy, kF32F64, false, sets},
                       {how->lambda, kF32F64, false, sets},
                       {data ? data->f : nullptr, kF32F64 | kU8, false, C},
                       {how->out_wx, kF32F64, true, sets},
                       {how->out_wy, kF32F64, true, sets},
                       {data ? data->out_lambda : nullptr, kF32F64, true, sets}};
    for (const auto &v : views)
        if (v.a) CCP_TRY(check_view(g, v.a, v.dtypes, v.output, 1, geo.H, geo.W, v.c));
    // an output that shares bytes with an input would be read by the neighbours' threads while its owner writes it
    for (int o = kInputs; o < kViews; ++o)
        for (int i = 0; i < kInputs && views[o].a; ++i) {
            if (!views[i].a) continue;
            uintptr_t olo, ohi, ilo, ihi;
            view_span(views[o].a, geo.H, geo.W, views[o].c, &olo, &ohi);
            view_span(views[i].a, geo.H, geo.W, views[i].c, &ilo, &ihi);
            if (olo < ihi && ilo < ohi) return CCP_ERR_BAD_ARG;
        }
    a->x = g->x.p;
    a->pitch = geo.pitch;
    a->W = geo.W;
    a->H = geo.H;
    a->cpb = C / sets;
    a->coupling = how->coupling;
    a->scale = how->scale;
    a->eps = how->epsilon;
    a->u = image_view(how->u, 0.0);
    a->gx = image_view(how->gx, 0.0);
    a->gy = image_view(how->gy, 0.0);
    a->bwx = image_view(how->base_wx, 1.0);
    a->bwy = image_view(how->base_wy, 1.0);
    a->lam = image_view(how->lambda, 0.0);
    a->out_wx = adj_out(how->out_wx);
    a->out_wy = adj_out(how->out_wy);
    return CCP_OK;
}

// Rows per strip of k_weighted_reweight_robust, by tools/robust_bench.py (NOTES R39.1 has the figures of 4, 8, 16 and 32 at
// both sizes): a tall strip forms fewer north weights twice, but a canvas cut into few strips leaves CUs without a block.
// At 4096^2 x 3 the pass was the faster the taller the strip (32: 16 x 128 blocks, 8 per CU of the 256), at 752 x 566 x 3 the
// slower (4: 3 x 142 blocks; 8 already leaves CUs idle and costs 28 %).  So: the tallest strip that still makes 8 blocks per
// CU, else 4.  CCP_GS_ROBUST_ROWS = 4 | 8 | 16 | 32 overrides it, for that measurement and for the tests of every strip
// height on small canvases; the bits do not depend on it.
int robust_rows(int W, int H, int sets)
{
    if (const char *e = getenv("CCP_GS_ROBUST_ROWS")) {
        const int r = atoi(e);
        if (r == 4 || r == 8 || r == 16 || r == 32) return r;
    }
    const long columns = (W + kBlock - 1) / kBlock, enough = 8 * 256;
    for (int r = 32; r > 4; r /= 2)
        if (columns * ((H + r - 1) / r) * sets >= enough) return r;
    return 4;
}

// ccp_grid_reweight_device (data: null) and ccp_grid_reweight_robust_device: refresh_device without a mask whose level-0 pass
// forms the weights (with `data`: lambda from |u - f| too, in the marching kernel)
int reweight_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data)
{
    RobustArgs a{};
    CCP_TRY(reweight_checked(g, how, data, &a.r));
    const Geom &geo = g->geom;
    const int sets = g->per_channel ? g->desc.channels : 1;
    const long n = geo.ch_stride;
    double *cons = g->has_fixed ? g->wcons.p : nullptr;
    if (!data)
        return refresh_pass(g, 1 + 3 * sets, [&] {
            with_phi(how->penalty, [&](auto P) {
                if constexpr (decltype(P)::value != kPhiQuadratic)           // (which reweight_checked refuses without `data`)
                    hipLaunchKernelGGL((k_weighted_reweight<decltype(P)::value>), pixels(geo.W, geo.H, sets), dim3(kBlock), 0, g->stream, a.r,
                                       g->wop.p, n, cons, g->rcount.p);
            });
        });
    a.rows = robust_rows(geo.W, geo.H, sets);
    a.dphi = data->penalty;
    a.dscale = data->scale;
    a.deps = data->penalty == CCP_REWEIGHT_QUADRATIC ? 1.0 : data->epsilon;   // (not read for QUADRATIC)
    a.f = image_view(data->f, 0.0);
    a.out_lam = adj_out(data->out_lambda);
    const dim3 grid((unsigned)((geo.W + kBlock - 1) / kBlock), (unsigned)((geo.H + a.rows - 1) / a.rows), (unsigned)sets);
    return refresh_pass(g, 1 + 3 * sets, [&] {
        with_phi(how->penalty, [&](auto P) {
            hipLaunchKernelGGL((k_weighted_reweight_robust<decltype(P)::value>), grid, dim3(kBlock), 0, g->stream, a, g->wop.p, n, cons,
                               g->rcount.p);
        });
    });
}

// ccp_grid_reweight_adjoint_device: the forward calls' checks on `how` and `data` with their outputs left out
// (reweight_checked), then the gradient views, and one launch of the marching kernel on the handle's stream.
int reweight_adjoint_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data, const ccp_reweight_grads *io)
{
    CCP_TRY(weighted_handle(g));
    if (!how || !io || !how->u) return CCP_ERR_BAD_ARG;
    if (!data && (io->grad_lambda || io->g_f || io->g_lambda)) return CCP_ERR_BAD_ARG;
    ccp_reweight fwd = *how;
    fwd.out_wx = fwd.out_wy = nullptr;                                     // ignored here
    ccp_reweight_data fwd_data{};
    if (data) {
        fwd_data = *data;
        fwd_data.out_lambda = nullptr;
    }
    ReweightAdjointArgs a{};
    CCP_TRY(reweight_checked(g, &fwd, data ? &fwd_data : nullptr, &a.f.r));
    const Geom &geo = g->geom;
    const int C = g->desc.channels, sets = g->per_channel ? C : 1;
    constexpr int kInputs = 10, kViews = 17;
    struct {
        const ccp_device_array *a;
        int c;
    } views[kViews] = {{how->u, C},          {how->gx, C},         {how->gy, C},        {how->base_wx, sets}, {how->base_wy, sets},
                       {how->lambda, sets},  {data ? data->f : nullptr, C},             {io->grad_wx, sets},  {io->grad_wy, sets},
                       {io->grad_lambda, sets}, {io->g_u, C},      {io->g_gx, C},       {io->g_gy, C},        {io->g_f, C},
                       {io->g_base_wx, sets}, {io->g_base_wy, sets}, {io->g_lambda, sets}};
    for (int i = 7; i < kViews; ++i)
        if (views[i].a) CCP_TRY(check_view(g, views[i].a, kF32F64, i >= kInputs, 1, geo.H, geo.W, views[i].c));
    // an output that shares bytes with an input or with another output: the neighbours' threads read the one, and two
    // stores to one address have no order
    for (int o = kInputs; o < kViews; ++o)
        for (int i = 0; i < kViews && views[o].a; ++i) {
            if (i == o || !views[i].a) continue;
            uintptr_t olo, ohi, ilo, ihi;
            view_span(views[o].a, geo.H, geo.W, views[o].c, &olo, &ohi);
            view_span(views[i].a, geo.H, geo.W, views[i].c, &ilo, &ihi);
            if (olo < ihi && ilo < ohi) return CCP_ERR_BAD_ARG;
        }
    a.f.rows = robust_rows(geo.W, geo.H, sets);
    a.f.dphi = data ? data->penalty : -1;
    a.f.dscale = data ? data->scale : 1.0;
    a.f.deps = data && data->penalty != CCP_REWEIGHT_QUADRATIC ? data->epsilon : 1.0;   // (not read for QUADRATIC)
    a.f.f = image_view(data ? data->f : nullptr, 0.0);
    a.grad_wx = image_view(io->grad_wx, 0.0);
    a.grad_wy = image_view(io->grad_wy, 0.0);
    a.grad_lam = image_view(io->grad_lambda, 0.0);
    a.g_u = adj_out(io->g_u);
    a.g_gx = adj_out(io->g_gx);
    a.g_gy = adj_out(io->g_gy);
    a.g_f = adj_out(io->g_f);
    a.g_bwx = adj_out(io->g_base_wx);
    a.g_bwy = adj_out(io->g_base_wy);
    a.g_lam = adj_out(io->g_lambda);
    const dim3 grid((unsigned)((geo.W + kBlock - 1) / kBlock), (unsigned)((geo.H + a.f.rows - 1) / a.f.rows), (unsigned)sets);
    with_phi(how->penalty, [&](auto P) {
        hipLaunchKernelGGL((k_weighted_reweight_adjoint<decltype(P)::value>), grid, dim3(kBlock), 0, g->stream, a, geo.ch_stride);
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// ccp_grid_irls_adjoint_step_device: the reweight adjoint's checks on `how` and `data`, then G, the mask and the report, then
// that ccp_grid_mg_prepare's work stands (b and x are the solve's); two launches on the handle's stream (one without a
// report).  The blocks' partial sums go to the handle's `partial`, which no weighted solve reads across calls.
int irls_adjoint_step_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data, const ccp_irls_adjoint_step *step)
{
    CCP_TRY(weighted_handle(g));
    if (!how || !step || !how->u || !step->grad_x) return CCP_ERR_BAD_ARG;
    ccp_reweight fwd = *how;
    fwd.out_wx = fwd.out_wy = nullptr;                                     // ignored here
    ccp_reweight_data fwd_data{};
    if (data) {
        fwd_data = *data;
        fwd_data.out_lambda = nullptr;
    }
    IrlsAdjointArgs a{};
    CCP_TRY(reweight_checked(g, &fwd, data ? &fwd_data : nullptr, &a.f.r));
    const Geom &geo = g->geom;
    const int C = g->desc.channels, sets = g->per_channel ? C : 1;
    CCP_TRY(check_view(g, step->grad_x, kF32F64, false, 1, geo.H, geo.W, C));
    if (step->fixed) CCP_TRY(check_view(g, step->fixed, kF32F64 | kU8, false, 1, geo.H, geo.W, sets));
    if (step->report) CCP_TRY(check_view(g, step->report, 1u << CCP_DTYPE_F64, true, 1, C, 2, 1));
    CCP_TRY(mg_prepared(g));
    a.f.rows = robust_rows(geo.W, geo.H, sets);
    const dim3 grid((unsigned)((geo.W + kBlock - 1) / kBlock), (unsigned)((geo.H + a.f.rows - 1) / a.f.rows), (unsigned)sets);
    const long blocks = (long)grid.x * grid.y;
    if (step->report && (size_t)(2 * C * blocks) > g->partial.n) return CCP_ERR_STATE;   // (the handle sizes it by rows, not strips)
    a.f.dphi = data ? data->penalty : -1;
    a.f.dscale = data ? data->scale : 1.0;
    a.f.deps = data && data->penalty != CCP_REWEIGHT_QUADRATIC ? data->epsilon : 1.0;   // (not read for QUADRATIC)
    a.f.f = image_view(data ? data->f : nullptr, 0.0);
    a.v = g->x.p;
    a.b = g->b.p;
    a.d = g->wop.p;
    a.plane = geo.ch_stride;
    a.dset = g->per_channel ? 4 * geo.ch_stride : 0;
    a.grad = image_view(step->grad_x, 0.0);
    a.fixed = image_view(step->fixed, 0.0);
    a.part = step->report ? g->partial.p : nullptr;
    with_phi(how->penalty, [&](auto P) {
        hipLaunchKernelGGL((k_irls_adjoint_step<decltype(P)::value>), grid, dim3(kBlock), 0, g->stream, a);
    });
    CCP_HIP(hipGetLastError());
    if (step->report) {
        hipLaunchKernelGGL(k_irls_adjoint_report, dim3((unsigned)C), dim3(kBlock), 0, g->stream, g->partial.p, blocks,
                           static_cast<double *>(const_cast<void *>(step->report->data)), (long)step->report->stride_y,
                           (long)step->report->stride_x);
        CCP_HIP(hipGetLastError());
    }
    return CCP_OK;
}

}  // namespace

int ccp::weighted_apply(ccp_grid *g, int mode) { return mode == 0 ? weighted_apply_mode<0>(g) : weighted_apply_mode<1>(g); }

extern "C" {

int ccp_grid_assemble_weighted_rhs(ccp_grid *g, const float *gx, const float *gy, int64_t field_stride_bytes, const float *f,
                                   int64_t f_stride_bytes, int32_t init_x_from_f)
try {
    CCP_TRY(weighted_handle(g));
    return weighted_rhs_host(g, gx, gy, field_stride_bytes, f, f_stride_bytes, nullptr, 0, init_x_from_f != 0);
} CCP_ABI_CATCH

int ccp_grid_assemble_weighted_rhs_device(ccp_grid *g, const ccp_device_array *gx, const ccp_device_array *gy, const ccp_device_array *f,
                                          int32_t init_x_from_f)
try {
    CCP_TRY(weighted_handle(g));
    return weighted_rhs_device(g, gx, gy, f, nullptr, init_x_from_f != 0);
} CCP_ABI_CATCH

int ccp_grid_assemble_constrained_rhs(ccp_grid *g, const float *gx, const float *gy, int64_t field_stride_bytes, const float *f,
                                      int64_t f_stride_bytes, const float *values, int64_t values_stride_bytes, int32_t init)
try {
    CCP_TRY(weighted_handle(g));
    return weighted_rhs_host(g, gx, gy, field_stride_bytes, f, f_stride_bytes, values, values_stride_bytes, init != 0);
} CCP_ABI_CATCH

int ccp_grid_assemble_constrained_rhs_device(ccp_grid *g, const ccp_device_array *gx, const ccp_device_array *gy, const ccp_device_array *f,
                                             const ccp_device_array *values, int32_t init)
try {
    CCP_TRY(weighted_handle(g));
    return weighted_rhs_device(g, gx, gy, f, values, init != 0);
} CCP_ABI_CATCH

int ccp_grid_set_weights_host(ccp_grid *g, const float *wx, const float *wy, const float *lambda, int64_t row_stride_bytes)
try {
    return ccp_grid_set_weights_constrained_host(g, wx, wy, lambda, row_stride_bytes, nullptr, 0);
} CCP_ABI_CATCH

int ccp_grid_set_weights_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda)
try {
    return ccp_grid_set_weights_constrained_device(g, wx, wy, lambda, nullptr);
} CCP_ABI_CATCH

int ccp_grid_set_weights_constrained_host(ccp_grid *g, const float *wx, const float *wy, const float *lambda, int64_t row_stride_bytes,
                                          const uint8_t *fixed, int64_t fixed_stride_bytes)
try {
    CCP_TRY(weighted_handle(g));
    const int W = g->desc.width, H = g->desc.height;
    const float *src[3] = {wx, wy, lambda};
    if ((wx || wy || lambda) && row_stride_bytes < (int64_t)W * (int64_t)sizeof(float)) return CCP_ERR_BAD_ARG;
    if (fixed && fixed_stride_bytes < (int64_t)W) return CCP_ERR_BAD_ARG;
    const double dflt[3] = {1.0, 1.0, 0.0};
    DevBuf<float> dev[3];
    DevBuf<uint8_t> dfix;
    ImageView v[3];
    for (int i = 0; i < 3; ++i) {
        v[i] = ImageView{nullptr, 0, 0, 0, 0, dflt[i]};
        if (!src[i]) continue;
        CCP_TRY(dev[i].alloc((size_t)W * H));
        CCP_HIP(hipMemcpy2DAsync(dev[i].p, (size_t)W * sizeof(float), src[i], (size_t)row_stride_bytes, (size_t)W * sizeof(float), (size_t)H,
                                 hipMemcpyHostToDevice, g->stream));
        v[i] = ImageView{dev[i].p, (long)W, 1, 0, CCP_DTYPE_F32, dflt[i]};
    }
    if (!fixed) return form_operator(g, false, v[0], v[1], v[2], nullptr);
    CCP_TRY(dfix.alloc((size_t)W * H));
    CCP_HIP(hipMemcpy2DAsync(dfix.p, (size_t)W, fixed, (size_t)fixed_stride_bytes, (size_t)W, (size_t)H, hipMemcpyHostToDevice, g->stream));
    const ImageView m{dfix.p, (long)W, 1, 0, CCP_DTYPE_U8, 0.0};
    return form_operator(g, false, v[0], v[1], v[2], &m);
} CCP_ABI_CATCH

int ccp_grid_set_weights_constrained_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                                            const ccp_device_array *fixed)
try {
    return set_weights_device(g, false, wx, wy, lambda, fixed);
} CCP_ABI_CATCH

int ccp_grid_constraint_info(ccp_grid *g, int64_t *fixed_pixels, int64_t *free_live_pixels, int64_t *boundary_edges)
try {
    return ccp_grid_constraint_info_channel(g, 0, fixed_pixels, free_live_pixels, boundary_edges);
} CCP_ABI_CATCH

int ccp_grid_constraint_info_channel(ccp_grid *g, int32_t channel, int64_t *fixed_pixels, int64_t *free_live_pixels, int64_t *boundary_edges)
try {
    CCP_TRY(weighted_handle(g));
    if (channel < 0 || channel >= g->desc.channels) return CCP_ERR_BAD_ARG;
    if (!g->has_op) return CCP_ERR_STATE;
    const int k = g->per_channel ? channel : 0;                            // the shared operator is every channel's
    if (g->refreshed) CCP_TRY(refreshed_counts(g));
    // an operator formed without a mask: its dead pixels counted once
    if (g->pc_live[k] < 0) CCP_TRY(count_live(g, g->wop.p + 4 * (long)k * g->geom.ch_stride, &g->pc_live[k]));
    if (fixed_pixels) *fixed_pixels = g->pc_fixed[k];
    if (free_live_pixels) *free_live_pixels = g->pc_live[k];
    if (boundary_edges) *boundary_edges = g->pc_edges[k];
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_weights_per_channel_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                                            const ccp_device_array *fixed)
try {
    return set_weights_device(g, true, wx, wy, lambda, fixed);
} CCP_ABI_CATCH

int ccp_grid_refresh_weights_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda)
try {
    return refresh_device(g, wx, wy, lambda, nullptr, false);
} CCP_ABI_CATCH

int ccp_grid_refresh_constrained_device(ccp_grid *g, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                                        const ccp_device_array *fixed)
try {
    return refresh_device(g, wx, wy, lambda, fixed, true);
} CCP_ABI_CATCH

int ccp_grid_reweight_device(ccp_grid *g, const ccp_reweight *how)
try {
    return reweight_device(g, how, nullptr);
} CCP_ABI_CATCH

int ccp_grid_reweight_robust_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data)
try {
    if (!data) return CCP_ERR_BAD_ARG;
    return reweight_device(g, how, data);
} CCP_ABI_CATCH

int ccp_grid_reweight_adjoint_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data, const ccp_reweight_grads *io)
try {
    return reweight_adjoint_device(g, how, data, io);
} CCP_ABI_CATCH

int ccp_grid_irls_adjoint_step_device(ccp_grid *g, const ccp_reweight *how, const ccp_reweight_data *data, const ccp_irls_adjoint_step *step)
try {
    return irls_adjoint_step_device(g, how, data, step);
} CCP_ABI_CATCH

int ccp_grid_reserve_constraints(ccp_grid *g, int32_t on)
try {
    CCP_TRY(weighted_handle(g));
    if (g->desc.ghost != 0 || g->desc.row_count < g->desc.height) return CCP_ERR_UNSUPPORTED;   // a row block
    g->reserve_cons = on != 0;                                             // the next setter's business: nothing changes now
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_operator_status(ccp_grid *g, int32_t *status)
try {
    CCP_TRY(weighted_handle(g));
    if (!status) return CCP_ERR_BAD_ARG;
    if (!g->has_op) return CCP_ERR_STATE;
    unsigned word = 0;
    if (g->refreshed) CCP_HIP(hipMemcpyAsync(&word, g->op_status.p, sizeof(word), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    *status = (int32_t)word;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_operator_channels(ccp_grid *g, int32_t *n)
try {
    CCP_TRY(weighted_handle(g));
    if (!n) return CCP_ERR_BAD_ARG;
    if (!g->has_op) return CCP_ERR_STATE;
    *n = g->per_channel ? g->desc.channels : 1;
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"

// ============================================================================================
// The backward pass of a weighted solve (include/ccp_gs.h, "Differentiating a weighted solve"; kernels: ccp_grid_adjoint.hpp)
// ============================================================================================
namespace {

AdjIn adj_in(const ccp_device_array *a)
{
    if (!a) return AdjIn{nullptr, 0, 0, 0, 0};
    return AdjIn{a->data, (long)a->stride_y, (long)a->stride_x, (long)a->stride_c, a->dtype};
}

AdjOut adj_out(const ccp_device_array *a)
{
    if (!a) return AdjOut{nullptr, 0, 0, 0, 0};
    return AdjOut{const_cast<void *>(a->data), (long)a->stride_y, (long)a->stride_x, (long)a->stride_c, a->dtype};
}

// channel c of a view as a one-channel view (one operator per channel: a launch per channel, each the launch of a
// one-channel handle on the channel's slices)
template <typename A>
A adj_channel(A a, int c)
{
    if (a.p) a.p = (decltype(a.p))((const char *)a.p + (long)c * a.sc * (long)dtype_bytes(a.dtype));
    return a;
}

}  // namespace

extern "C" {

int ccp_grid_adjoint_begin_device(ccp_grid *g, const ccp_device_array *grad_x)
try {
    CCP_TRY(weighted_handle(g));
    const Geom &geo = g->geom;
    CCP_TRY(check_view(g, grad_x, kF32F64, false, 1, geo.H, geo.W, g->desc.channels));
    if (!g->has_op) return CCP_ERR_STATE;
    if (g->per_channel) {                                                    // channel c's free / live set: its own d
        const long n = geo.ch_stride;
        for (int c = 0; c < g->desc.channels; ++c) {
            hipLaunchKernelGGL(k_adjoint_begin, pixel_grid(g, geo.H), dim3(kBlock), 0, g->stream, g->b.p + c * n, g->x.p + c * n,
                               g->wop.p + 4 * c * n, geo.pitch, n, geo.W, 1, adj_channel(adj_in(grad_x), c));
            CCP_HIP(hipGetLastError());
        }
        return edge_timeout_status(g);
    }
    hipLaunchKernelGGL(k_adjoint_begin, pixel_grid(g, geo.H), dim3(kBlock), 0, g->stream, g->b.p, g->x.p, g->wop.p, geo.pitch, geo.ch_stride,
                       geo.W, g->desc.channels, adj_in(grad_x));
    CCP_HIP(hipGetLastError());
    return edge_timeout_status(g);
} CCP_ABI_CATCH

int ccp_grid_weighted_adjoint_device(ccp_grid *g, const ccp_adjoint_inputs *in, const ccp_adjoint_outputs *out)
try {
    CCP_TRY(weighted_handle(g));
    if (!in || !out) return CCP_ERR_BAD_ARG;
    const Geom &geo = g->geom;
    const int W = geo.W, H = geo.H, C = g->desc.channels;
    CCP_TRY(check_view(g, in->u, 1u << CCP_DTYPE_F64, false, 1, H, W, C));
    if (in->grad_x || out->g_values) CCP_TRY(check_view(g, in->grad_x, kF32F64, false, 1, H, W, C));
    if (in->gx) CCP_TRY(check_view(g, in->gx, kF32, false, 1, H, W, C));
    if (in->gy) CCP_TRY(check_view(g, in->gy, kF32, false, 1, H, W, C));
    if (in->f) CCP_TRY(check_view(g, in->f, kF32F64 | kU8, false, 1, H, W, C));
    const int PC = g->has_op && g->per_channel ? C : 1;                      // the extent of the weight views along c
    if (in->wx) CCP_TRY(check_view(g, in->wx, kF32F64, false, 1, H, W, PC));
    if (in->wy) CCP_TRY(check_view(g, in->wy, kF32F64, false, 1, H, W, PC));
    if (in->lambda) CCP_TRY(check_view(g, in->lambda, kF32F64, false, 1, H, W, PC));
    if (in->fixed) CCP_TRY(check_view(g, in->fixed, kF32F64 | kU8, false, 1, H, W, PC));
    const ccp_device_array *planes[3] = {out->g_wx, out->g_wy, out->g_lambda};
    const ccp_device_array *images[4] = {out->g_gx, out->g_gy, out->g_f, out->g_values};
    for (const ccp_device_array *a : planes)
        if (a) CCP_TRY(check_view(g, a, kF32F64, true, 1, H, W, PC));
    for (const ccp_device_array *a : images)
        if (a) CCP_TRY(check_view(g, a, kF32F64, true, 1, H, W, C));
    if (!g->has_op) return CCP_ERR_STATE;
    AdjointArgs a{};
    a.v = g->x.p;
    a.pitch = geo.pitch;
    a.ch_stride = geo.ch_stride;
    a.W = W;
    a.H = H;
    a.C = C;
    a.u = adj_in(in->u);
    a.grad = adj_in(in->grad_x);
    a.gx = adj_in(in->gx);
    a.gy = adj_in(in->gy);
    a.f = adj_in(in->f);
    a.wx = adj_in(in->wx);
    a.wy = adj_in(in->wy);
    a.lam = adj_in(in->lambda);
    a.fixed = adj_in(in->fixed);
    a.g_wx = adj_out(out->g_wx);
    a.g_wy = adj_out(out->g_wy);
    a.g_lam = adj_out(out->g_lambda);
    a.g_gx = adj_out(out->g_gx);
    a.g_gy = adj_out(out->g_gy);
    a.g_f = adj_out(out->g_f);
    a.g_val = adj_out(out->g_values);
    if (g->per_channel) {
        // H x W x C weights and weight gradients (their stride_c is used), no sum over channels: one launch per channel,
        // each the launch of a one-channel handle on channel c's slice of every view
        for (int c = 0; c < C; ++c) {
            AdjointArgs k = a;
            k.C = 1;
            k.v = a.v + (long)c * geo.ch_stride;
            k.u = adj_channel(a.u, c);
            k.grad = adj_channel(a.grad, c);
            k.gx = adj_channel(a.gx, c);
            k.gy = adj_channel(a.gy, c);
            k.f = adj_channel(a.f, c);
            k.wx = adj_channel(a.wx, c);
            k.wy = adj_channel(a.wy, c);
            k.lam = adj_channel(a.lam, c);
            k.fixed = adj_channel(a.fixed, c);
            k.g_wx = adj_channel(a.g_wx, c);
            k.g_wy = adj_channel(a.g_wy, c);
            k.g_lam = adj_channel(a.g_lam, c);
            k.g_gx = adj_channel(a.g_gx, c);
            k.g_gy = adj_channel(a.g_gy, c);
            k.g_f = adj_channel(a.g_f, c);
            k.g_val = adj_channel(a.g_val, c);
            hipLaunchKernelGGL(k_weighted_adjoint, pixel_grid(g, H), dim3(kBlock), 0, g->stream, k);
            CCP_HIP(hipGetLastError());
        }
        return edge_timeout_status(g);
    }
    a.wx.sc = a.wy.sc = a.lam.sc = a.fixed.sc = 0;         // H x W: stride_c unused
    a.g_wx.sc = a.g_wy.sc = a.g_lam.sc = 0;
    hipLaunchKernelGGL(k_weighted_adjoint, pixel_grid(g, H), dim3(kBlock), 0, g->stream, a);
    CCP_HIP(hipGetLastError());
    return edge_timeout_status(g);
} CCP_ABI_CATCH

}  // extern "C"
