// ccp_grid_mg.hip — multigrid-preconditioned conjugate gradient on the grid handles (include/ccp_gs.h:
// ccp_grid_mg_*).  Kernels and the algorithm: ccp_grid_mg.hpp.
#include "ccp_grid_mg.hpp"
#include "ccp_grid_mgs.hpp"
#include "ccp_grid_mgb.hpp"
#include "ccp_grid_mgl.hpp"
#include "ccp_grid_mgn.hpp"
#include "ccp_grid_mge.hpp"
#include "ccp_grid_mgr.hpp"
#include "ccp_view_check.hpp"
#include "ccp_grid_weighted_api.hpp"
#include "ccp_comm.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <type_traits>
#include <vector>

using namespace ccp;

namespace ccp {

// The work set of a PCG over C channels: z, r, p, ap (C x n doubles each, zero-filled), C slices of `ps` partial sums
// and CgState[C].
struct PcgWork {
    DevBuf<double> z, r, p, ap, partial;
    DevBuf<CgState> state;
    long ps = 0;                     // partial sums per channel
    // What is not there yet: the vectors; with partial_per_channel > 0 the partial sums and the states too (a V-cycle
    // on row blocks needs the vectors alone).
    int alloc(int C, long n, long partial_per_channel, hipStream_t s)
    {
        if (!ap.p)                                                  // (the last one made: all four are there or none is used)
            for (DevBuf<double> *v : {&z, &r, &p, &ap}) {
                CCP_TRY(v->alloc((size_t)(C * n)));
                CCP_HIP(hipMemsetAsync(v->p, 0, sizeof(double) * C * n, s));
            }
        if (partial_per_channel > 0 && !state.p) {
            ps = partial_per_channel;
            CCP_TRY(partial.alloc((size_t)(C * ps)));
            CCP_TRY(state.alloc((size_t)C));
        }
        return CCP_OK;
    }
    void release()
    {
        for (DevBuf<double> *v : {&z, &r, &p, &ap, &partial}) v->release();
        state.release();
        ps = 0;
    }
};

// The hierarchy of one handle: level 0 is the handle's own operator and vectors; levels 1.. own d, we, ws, b, z in
// one allocation (level layout, pads zero; a weighted hierarchy adds lambda).  The PCG work sets (`seq`: one channel,
// `bat`: all of them) are allocated at the first solve of their mode.
// Row blocks (ccp_grid_mg_conjugate_gradient_rowblocked): levels 0 .. dist-1 hold the block's own rows plus up to
// kMgGhost ghost rows per neighbour side (level 0 in a layout of its own: the MG vectors do not depend on the
// handle's ghost depth); every level from `dist` on is held whole by every rank.
struct MgHierarchy {
    int levels = 0;
    int tail = 0;                    // first level of k_mg_tail (>= 1), or `levels` for a one-level hierarchy
    bool rowblocked = false;
    int dist = 0;                    // row blocks: the number of distributed levels (>= 1)
    std::vector<std::vector<int>> own;   // row blocks, per distributed level: every rank's first global row, then H_k
    DevBuf<unsigned char> mask0;     // row blocks: level 0's mask in the level's layout
    std::vector<MgLevel> lv;
    std::vector<long> base;          // per coarse level: offset of its d in `store` (then we, ws, b, z, t, [lambda], each `size`)
    std::vector<long> size;
    DevBuf<double> store;
    DevBuf<double> t0;               // level 0's pre-smoothed z (one channel): k_mg_tile reads it while it writes z
    PcgWork seq;                     // the sequential mode and the row-block calls (there n is level 0's, ghost rows included)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int kind0 = kMgSolve;
    bool weighted = false;           // level 0 is a weighted handle's stored operator; every level carries lambda (arr 6)
    double cs = 2.0;                 // the coarse correction's scale (`cs` of k_mg_tile, k_mg_tail): 1.0 on a rescaled weighted hierarchy
    // CCP_MG_PRECISION_F32 (ccp_grid_mgs.hpp): the narrowed coefficients and the float vectors of the V-cycle, made at the
    // first V-cycle (narrow_levels).  fstore: per coarse level d, we, ws, b, z, t, each `size` floats; w32: a weighted
    // handle's level-0 d, we, ws; t0f: level 0's pre-smoothed z (the fp64 t0 is not allocated then).
    int precision = CCP_MG_PRECISION_F64;
    int narrowed = 0;                // 0: not yet, 1: ready, -1: refused (a coefficient does not narrow to a usable float)
    std::vector<MgsLevel> flv;
    std::vector<long> fbase;
    DevBuf<float> fstore, w32, t0f;
    DevBuf<unsigned> fbad;
    // one operator (opC == 1) only: 0 d, 1 we, 2 ws, 3 b, 4 z, 5 t.  Code that may see opC > 1 asks fcoef() / fvec().
    float *farr(int k, int which) { return fstore.p + fbase[k] + (long)which * size[k]; }
    int lam_slot = 6;                // F32: 3 (the fp64 store then holds d, we, ws and lambda only)
    // CCP_MG_CHANNELS_BATCHED (ccp_grid_mgb.hpp): C of every vector, made at the first batched V-cycle (bt0: level 0's t;
    // bstore: per coarse level b, z, t, each C x `size`) and at the first batched solve (the work set `bat`).  The levels'
    // coefficients are shared with the sequential mode.
    int bC = 0;
    std::vector<long> bbase;
    DevBuf<double> bt0, bstore;
    PcgWork bat;
    double *barr(int k, int which) { return bstore.p + bbase[k] + (long)which * bC * size[k]; }   // 0 b, 1 z, 2 t: channel ch at + ch * size[k]
    // CCP_MG_SMOOTHER_LINE (ccp_grid_mgl.hpp): the smoother of the levels above the tail, taken from the handle at every
    // call (hierarchy: whole_levels is handed the hierarchy by the steps objects, which know no view), and the three work
    // planes of the line solves, made at the first line V-cycle (line_planes): each as long as the largest level above
    // the tail, lwork holds them one after the other.
    int smoother = CCP_MG_SMOOTHER_POINT;
    long lplane = 0;
    DevBuf<double> lwork;
    // CCP_MG_NULLSPACE_CONSTANT (ccp_grid_mgn.hpp), made at the first call in that mode: the census counts (one word per
    // operator), the solve's device scalars and the partial sums of its three-sum reduction (3 x 2,048)
    DevBuf<unsigned> nscount;
    DevBuf<MgnState> nsstate;        // one per channel: read back once, after the last channel's solve
    DevBuf<double> nspart;
    // ccp_grid_mg_prepare / ccp_grid_mg_conjugate_gradient_enqueue (ccp_grid_mge.hpp): the enqueue solve's states, one per
    // channel in either channel mode (the report kernel reads them all after the last channel), and what the last
    // successful prepare built for (prepared_for) -- the enqueue call runs only on exactly that.  Everything else prepare
    // builds is what the synchronous solve builds at its first call; a setter that frees part of it clears `prepared`
    // (kOptions).
    DevBuf<CgState> estate;
    // ccp_grid_mg_conjugate_gradient_enqueue_relative (ccp_grid_mgr.hpp), made by every prepare: kMaxChannels thresholds,
    // kMaxChannels norms of b, then the partial sums of b'b (the solve's own count: one channel's, or C of them in batched mode)
    DevBuf<double> erel;
    bool prepared = false;
    MgConfig prep_cfg;
    int prep_nu = 0, prep_channels = 0;
    // one operator (opC == 1) only: 0 d, 1 we, 2 ws, 3 b, 4 z, 5 t, 6 lambda (lam_slot).  The one-block code, which may see
    // opC > 1, asks coef() for a coefficient plane and vec() for a vector; the row-block code (never weighted) uses arr().
    double *arr(int k, int which) { return store.p + base[k] + (long)which * size[k]; }
    // One operator per channel (a weighted handle after ccp_grid_set_weights_per_channel_device): opC
    // copies of the coefficient part of every level.  The coarse levels' d, we, ws, lambda of all channels live in cstore
    // (level k, channel ch: at cbase[k] + 4 ch size[k], each `size[k]`), the float copies of d, we, ws in cfstore (3 per
    // channel) and w32 (level 0, 3 n0 per channel); store and fstore then hold the vectors b, z, t alone (vec, fvec).
    // clv / cflv: every channel's level descriptors -- the same structs with the channel's pointers; the sequential
    // V-cycle and PCG are handed the channel and read levels_of(ch) / flevels_of(ch), nothing else.
    int opC = 1;
    long os0 = 0;                    // level 0's per-channel stride of d, we, ws (the handle's)
    DevBuf<MgTail> ctails;           // batched mode: every channel's tail descriptor (k_pco_tail), made with batched_levels
    std::vector<long> cbase;
    DevBuf<double> cstore;
    DevBuf<float> cfstore;
    std::vector<std::vector<MgLevel>> clv;
    std::vector<std::vector<MgsLevel>> cflv;
    // which: 0 d, 1 we, 2 ws, 3 lambda
    double *coef(int ch, int k, int which)
    {
        if (opC == 1) return arr(k, which == 3 ? lam_slot : which);
        return cstore.p + cbase[k] + (4L * ch + which) * size[k];
    }
    float *fcoef(int ch, int k, int which) { return opC == 1 ? farr(k, which) : cfstore.p + 3 * cbase[k] / 4 + (3L * ch + which) * size[k]; }
    // which: 0 b, 1 z, 2 t of coarse level k (one set: the sequential V-cycle's)
    double *vec(int k, int which) { return store.p + base[k] + (long)(opC == 1 ? 3 + which : which) * size[k]; }
    float *fvec(int k, int which) { return fstore.p + fbase[k] + (long)(opC == 1 ? 3 + which : which) * size[k]; }
    const std::vector<MgLevel> &levels_of(int ch) const { return opC == 1 ? lv : clv[(size_t)ch]; }
    const std::vector<MgsLevel> &flevels_of(int ch) const { return opC == 1 ? flv : cflv[(size_t)ch]; }
    ~MgHierarchy()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

void mg_release(MgHierarchy **cache)
{
    delete *cache;
    *cache = nullptr;
}

}  // namespace ccp

namespace {

dim3 cells_grid(int w, int h) { return dim3((unsigned)((w + kBlock - 1) / kBlock), (unsigned)h); }

// A level's run-time kind as a template argument: f(K) with decltype(K)::value == kind; returns what f returns.  A step
// that takes a bool too goes through with_bool (ccp_common.hpp) inside f.  (f is instantiated for all three kinds: where a kernel exists
// for fewer, as the fp32 V-cycle's coarse levels do for kMgCoarse alone, name the kind and do not come here.)
template <typename F>
auto with_kind(int kind, F &&f)
{
    if (kind == kMgCoarse) return f(std::integral_constant<int, kMgCoarse>{});
    else if (kind == kMgMasked) return f(std::integral_constant<int, kMgMasked>{});
    else return f(std::integral_constant<int, kMgSolve>{});
}

// coarse local rows [Y0, Y0 + rows) of c from f (kind: f's operator)
void coarsen(int kind, hipStream_t s, const MgLevel &f, const MgLevel &c, int Y0, int rows, double *d, double *we, double *ws)
{
    if (rows <= 0) return;
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_mg_coarsen<decltype(K)::value>), cells_grid(c.W, rows), dim3(kBlock), 0, s, f, c, Y0, d, we, ws);
    });
}

int level_kind(const MgHierarchy &h, int k) { return k ? kMgCoarse : h.kind0; }

// The hierarchy of a view laid out and allocated, every buffer zeroed, its coarse levels not filled yet: build's first half
int lay_out(const GridMgView &v, MgHierarchy **out)
{
    MgHierarchy *h = new MgHierarchy();
    std::unique_ptr<MgHierarchy> own(h);
    h->kind0 = v.weighted ? kMgCoarse : v.masked ? kMgMasked : kMgSolve;
    h->weighted = v.weighted;
    h->precision = v.cfg.precision;
    // (ccp_grid_mg_set_hierarchy drops the cached hierarchy when the kind changes: a cached one is of the handle's kind)
    const bool rescaled = v.weighted && v.cfg.hierarchy == CCP_MG_HIERARCHY_RESCALED;
    h->cs = rescaled ? 1.0 : 2.0;
    // per coarse level d, we, ws, the V-cycle's b, z, t, and a weighted handle's lambda; the fp32 V-cycle keeps its vectors
    // in float (narrow_levels), so its fp64 store holds the coefficients alone: what ccp_grid_mg_level returns and the
    // narrowing reads
    const bool f32 = v.cfg.precision == CCP_MG_PRECISION_F32;
    h->lam_slot = f32 ? 3 : 6;
    const int OC = v.weighted ? v.op_channels : 1;                  // operators: > 1 keeps the coefficients in cstore
    h->opC = OC;
    h->os0 = v.op_stride;
    const int per_level = OC > 1 ? (f32 ? 0 : 3) : (f32 ? 3 : 6) + (v.weighted ? 1 : 0);
    MgLevel l0{};
    l0.W = v.geom.W;
    l0.H = v.geom.H;
    l0.pitch = v.geom.pitch;
    l0.mask = v.mask;
    if (v.weighted) {
        l0.d = v.wd;
        l0.we = v.wwe;
        l0.ws = v.wws;
    }
    l0.g0 = v.geom;
    l0.hi = l0.H;
    h->lv.push_back(l0);
    h->base.push_back(0);
    h->size.push_back(0);
    h->cbase.push_back(0);
    long total = 0, ctotal = 0;
    while (h->lv.back().W > 1 || h->lv.back().H > 1) {
        MgLevel c{};
        c.W = (h->lv.back().W + 1) / 2;
        c.H = (h->lv.back().H + 1) / 2;
        c.pitch = (((long)c.W + 1) / 2 + 15) / 16 * 16;
        c.hi = c.H;
        h->lv.push_back(c);
        h->base.push_back(total);
        h->size.push_back((long)c.H * 2 * c.pitch);
        total += per_level * h->size.back();
        h->cbase.push_back(ctotal);
        ctotal += 4L * OC * h->size.back();
    }
    h->levels = (int)h->lv.size();
    h->tail = h->levels;
    for (int k = 1; k < h->levels; ++k)
        if (h->lv[k].W <= kMgTailSide && h->lv[k].H <= kMgTailSide) {
            h->tail = k;
            break;
        }
    if (h->levels - h->tail > kMgTailLevels) return CCP_ERR_STATE;     // (cannot happen: sides <= 32 leave <= 6 levels)
    if (OC > 1 && ctotal > 0) {
        CCP_TRY(h->cstore.alloc((size_t)ctotal));
        CCP_HIP(hipMemsetAsync(h->cstore.p, 0, sizeof(double) * ctotal, v.stream));
    }
    if (!f32) {                                                     // (the fp32 V-cycle keeps its own, in float: narrow_levels)
        CCP_TRY(h->t0.alloc((size_t)v.geom.ch_stride));
        CCP_HIP(hipMemsetAsync(h->t0.p, 0, sizeof(double) * v.geom.ch_stride, v.stream));
    }
    if (total > 0) {
        CCP_TRY(h->store.alloc((size_t)total));
        CCP_HIP(hipMemsetAsync(h->store.p, 0, sizeof(double) * total, v.stream));
    }
    for (int k = 1; k < h->levels; ++k) {
        h->lv[k].d = h->coef(0, k, 0);
        h->lv[k].we = h->coef(0, k, 1);
        h->lv[k].ws = h->coef(0, k, 2);
    }
    if (OC > 1) {                                                   // every channel's descriptors: lv with the channel's planes
        for (int ch = 0; ch < OC; ++ch) {
            h->clv.push_back(h->lv);
            std::vector<MgLevel> &l = h->clv.back();
            l[0].d = v.wd + ch * v.op_stride;
            l[0].we = v.wwe + ch * v.op_stride;
            l[0].ws = v.wws + ch * v.op_stride;
            for (int k = 1; k < h->levels; ++k) {
                l[k].d = h->coef(ch, k, 0);
                l[k].we = h->coef(ch, k, 1);
                l[k].ws = h->coef(ch, k, 2);
            }
        }
    }
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return CCP_ERR_HIP;
    *out = own.release();
    return CCP_OK;
}

// The coarse levels' coefficients from level 0, every cell of every level: launches only.  build's second half, and
// all the hierarchy's fp64 coefficients need of ccp_grid_refresh_weights_device.
int fill_levels(const GridMgView &v, MgHierarchy &h)
{
    const double edge = v.weighted && v.cfg.hierarchy == CCP_MG_HIERARCHY_RESCALED ? 0.5 : 1.0;
    for (int k = 0; k + 1 < h.levels; ++k) {
        if (v.weighted)                                             // level k + 1 of all opC operators in one launch
            CCP_TRY(weighted_coarsen(v.stream, h.opC, h.lv[k], k ? 4 * h.size[k] : v.op_stride,
                                     k ? static_cast<const double *>(h.coef(0, k, 3)) : v.wlam, k ? 4 * h.size[k] : v.lam_stride, h.lv[k + 1],
                                     h.coef(0, k + 1, 0), h.coef(0, k + 1, 1), h.coef(0, k + 1, 2), h.coef(0, k + 1, 3), 4 * h.size[k + 1], edge));
        else
            coarsen(level_kind(h, k), v.stream, h.lv[k], h.lv[k + 1], 0, h.lv[k + 1].H, h.arr(k + 1, 0), h.arr(k + 1, 1), h.arr(k + 1, 2));
        CCP_HIP(hipGetLastError());
    }
    return CCP_OK;
}

int build(const GridMgView &v, MgHierarchy **out)
{
    MgHierarchy *h = nullptr;
    CCP_TRY(lay_out(v, &h));
    const int st = fill_levels(v, *h);
    if (st != CCP_OK) {
        delete h;
        return st;
    }
    *out = h;
    return CCP_OK;
}

// Does the cached hierarchy h serve the one-block calls on this view?  (Not one built for the row-block calls, for
// another precision or for another set of operators; a change of the hierarchy kind has deleted it: kOptions.)
bool cache_serves(const GridMgView &v, const MgHierarchy &h)
{
    return !h.rowblocked && h.weighted == v.weighted && h.precision == v.cfg.precision && h.opC == (v.weighted ? v.op_channels : 1);
}

int hierarchy(const GridMgView &v, MgHierarchy **out)
{
    if (*v.cache && !cache_serves(v, **v.cache)) mg_release(v.cache);
    if (!*v.cache) CCP_TRY(build(v, v.cache));
    *out = *v.cache;
    (*out)->smoother = v.cfg.smoother;
    return CCP_OK;
}

// smoothing_sweeps 0: the smoother's default, 2 red-black sweeps or 1 line sweep
int sweeps_arg(int32_t smoothing_sweeps, int *nu, int smoother = CCP_MG_SMOOTHER_POINT)
{
    if (smoothing_sweeps < 0 || smoothing_sweeps > 4) return CCP_ERR_BAD_ARG;
    *nu = smoothing_sweeps == 0 ? (smoother == CCP_MG_SMOOTHER_LINE ? 1 : 2) : smoothing_sweeps;
    return CCP_OK;
}

// one level above the tail: pre-smoothing and restriction (down), prolongation and post-smoothing (up)

dim3 tiles(const MgLevel &f) { return dim3((unsigned)((f.W + kMgTileW - 1) / kMgTileW), (unsigned)((f.hi - f.lo + kMgTileH - 1) / kMgTileH)); }

// t: the level's pre-smoothed z (restriction and the post-smoothing pass read it), z: its correction.  grid: tiles(f),
// or one workgroup for a 1x1 image (there t = b/d, what red updates from z = 0 give, is the V-cycle's z).
void pre(int kind, hipStream_t s, dim3 grid, const MgLevel &f, const double *b, double *t, int nu, const CgState *st)
{
    const double *none = nullptr;
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_mg_tile<decltype(K)::value, false>), grid, dim3(kBlock), mg_tile_lds(nu), s, f, b, none, t, f, none, 2.0, nu, st);
    });
}

// coarse local rows [Y0, Y0 + rows) of bc from f's residual
void restrict_rows(int kind, hipStream_t s, const MgLevel &f, const double *b, const double *t, const MgLevel &c, int Y0, int rows,
                   double *bc, const CgState *st)
{
    if (rows <= 0) return;
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_mg_restrict<decltype(K)::value>), cells_grid(c.W, rows), dim3(kBlock), 0, s, f, b, t, c, Y0, bc, st);
    });
}

// cs: the scale of the coarse correction (MgHierarchy::cs)
void post(int kind, hipStream_t s, const MgLevel &f, const double *b, const double *t, double *z, const MgLevel &c, const double *ec, double cs,
          int nu, const CgState *st)
{
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_mg_tile<decltype(K)::value, true>), tiles(f), dim3(kBlock), mg_tile_lds(nu), s, f, b, t, z, c, ec, cs, nu, st);
    });
}

// ---- CCP_MG_SMOOTHER_LINE (ccp_grid_mgl.hpp) ---------------------------------------------------------------------------
// the work planes of the line solves, once per hierarchy (what the line mode serves: config_check)
int line_planes(const GridMgView &v, MgHierarchy &h)
{
    if (v.cfg.smoother != CCP_MG_SMOOTHER_LINE || h.lwork.p) return CCP_OK;
    long n = 0;
    // level 0 is indexed by mg_at(pitch, x, y) < H * 2 * pitch, which is ch_stride on a weighted handle (one block, no ghost rows)
    for (int k = 0; k < h.tail && k < h.levels; ++k) n = std::max(n, k ? h.size[k] : (long)v.geom.ch_stride);
    CCP_TRY(h.lwork.alloc((size_t)(3 * n)));                       // (not cleared: a lane reads only what it wrote in the same launch)
    h.lplane = n;
    return CCP_OK;
}

// one half pass: the lines of direction DIR and parity `parity` of level f
template <int DIR, bool FIRST, bool ADD>
void lines(MgHierarchy &h, hipStream_t s, const MgLevel &f, const double *b, const double *z_in, double *z_out, const MgLevel &c,
           const double *ec, double cs, int parity, const CgState *st)
{
    const int n = DIR == kMglX ? f.W : f.H, across = DIR == kMglX ? f.H : f.W;
    const int count = (across - parity + 1) / 2;                   // lines of this parity
    if (count <= 0) return;
    const int L = mgl_lanes(DIR, n), per = kBlock / L;
    double *w = h.lwork.p;
    hipLaunchKernelGGL((k_mgl_lines<DIR, FIRST, ADD>), dim3((unsigned)((count + per - 1) / per)), dim3(kBlock), 0, s, f, b, z_in, z_out, w,
                       w + h.lplane, w + 2 * h.lplane, c, ec, cs, parity, L, st);
}

// nu line sweeps from t = 0, in place: x even (the first one from b alone), x odd, y even, y odd
void pre_lines(MgHierarchy &h, hipStream_t s, const MgLevel &f, const double *b, double *t, int nu, const CgState *st)
{
    const double *none = nullptr;
    for (int i = 0; i < nu; ++i) {
        if (i == 0) lines<kMglX, true, false>(h, s, f, b, t, t, f, none, 0.0, 0, st);
        else lines<kMglX, false, false>(h, s, f, b, t, t, f, none, 0.0, 0, st);
        lines<kMglX, false, false>(h, s, f, b, t, t, f, none, 0.0, 1, st);
        lines<kMglY, false, false>(h, s, f, b, t, t, f, none, 0.0, 0, st);
        lines<kMglY, false, false>(h, s, f, b, t, t, f, none, 0.0, 1, st);
    }
}

// z = t + cs e_c, then nu line sweeps in the reverse order: y odd (reads t + cs e_c, writes z), y even, x odd, x even
void post_lines(MgHierarchy &h, hipStream_t s, const MgLevel &f, const double *b, const double *t, double *z, const MgLevel &c,
                const double *ec, double cs, int nu, const CgState *st)
{
    const double *none = nullptr;
    for (int i = 0; i < nu; ++i) {
        if (i == 0) lines<kMglY, false, true>(h, s, f, b, t, z, c, ec, cs, 1, st);
        else lines<kMglY, false, false>(h, s, f, b, z, z, f, none, 0.0, 1, st);
        lines<kMglY, false, false>(h, s, f, b, z, z, f, none, 0.0, 0, st);
        lines<kMglX, false, false>(h, s, f, b, z, z, f, none, 0.0, 1, st);
        lines<kMglX, false, false>(h, s, f, b, z, z, f, none, 0.0, 0, st);
    }
}

// The tail kernels' descriptor (MgTail of MgLevel, MgsTail of MgsLevel): the levels from `first` on, their cells packed
// one level after the other.
template <typename Tail, typename Level>
Tail tail_of(const std::vector<Level> &lv, int first)
{
    Tail t{};
    t.levels = (int)lv.size() - first;
    int off = 0;
    for (int i = 0; i < t.levels; ++i) {
        const Level &l = lv[first + i];
        t.W[i] = l.W;
        t.H[i] = l.H;
        t.pitch[i] = l.pitch;
        t.off[i] = off;
        t.d[i] = l.d;
        t.we[i] = l.we;
        t.ws[i] = l.ws;
        off += l.W * l.H;
    }
    return t;
}

// The levels from `from` (held whole) down: tiles above the tail, then k_mg_tail, then back up to `from`.  Every launch
// is a no-op once st->active is 0 (st may be null).
// ch: whose operator (one operator per channel; 0 otherwise).
int whole_levels(MgHierarchy &h, hipStream_t s, int from, const double *b0, double *z0, int nu, const CgState *st, int ch = 0)
{
    const std::vector<MgLevel> &lv = h.levels_of(ch);
    auto B = [&](int k) -> const double * { return k ? h.vec(k, 0) : b0; };
    auto Z = [&](int k) -> double * { return k ? h.vec(k, 1) : z0; };
    auto T = [&](int k) -> double * { return k ? h.vec(k, 2) : h.t0.p; };
    const bool line = h.smoother == CCP_MG_SMOOTHER_LINE;
    for (int k = from; k < h.tail; ++k) {
        if (line) pre_lines(h, s, lv[k], B(k), T(k), nu, st);
        else pre(level_kind(h, k), s, tiles(lv[k]), lv[k], B(k), T(k), nu, st);
        restrict_rows(level_kind(h, k), s, lv[k], B(k), T(k), lv[k + 1], 0, lv[k + 1].H, h.vec(k + 1, 0), st);
    }
    const MgTail t = tail_of<MgTail>(lv, h.tail);
    hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(kBlock), 0, s, t, B(h.tail), Z(h.tail), h.cs, nu, st);
    for (int k = h.tail - 1; k >= from; --k) {
        if (line) post_lines(h, s, lv[k], B(k), T(k), Z(k), lv[k + 1], h.vec(k + 1, 1), h.cs, nu, st);
        else post(level_kind(h, k), s, lv[k], B(k), T(k), Z(k), lv[k + 1], h.vec(k + 1, 1), h.cs, nu, st);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// ---- CCP_MG_PRECISION_F32 (ccp_grid_mgs.hpp) -------------------------------------------------------------------------
// The narrowing itself: every level's d, we, ws of every operator into its float copy, every launch ORing into h.fbad,
// which the caller has cleared (narrow_levels by a memset; ccp_grid_refresh_weights_device, which runs these launches
// again on new values, in k_mge_clear).  Launches only.
int narrow_launch(const GridMgView &v, MgHierarchy &h)
{
    hipStream_t s = v.stream;
    const long n0 = v.geom.ch_stride;
    auto narrow = [&](const double *src, float *dst, long n) {
        hipLaunchKernelGGL(k_mgs_narrow, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, src, dst, n, h.fbad.p);
    };
    for (int ch = 0; ch < h.opC; ++ch)
        for (int k = 0; k < h.levels; ++k) {
            if (k) narrow(h.coef(ch, k, 0), h.fcoef(ch, k, 0), 3 * h.size[k]);   // d, we, ws lie one after the other in both stores
            else if (h.weighted) narrow(h.levels_of(ch)[0].d, h.w32.p + 3 * n0 * ch, 3 * n0);   // the handle's planes, n0 doubles apart
        }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// The float copies of every level's coefficients and the float vectors, once per hierarchy: allocated and described
// here, filled by narrow_launch.  CCP_ERR_UNSUPPORTED (now and at every later V-cycle of this hierarchy) if a coefficient
// narrows to inf or a non-zero one to 0.  One read-back.
int narrow_levels(const GridMgView &v, MgHierarchy &h)
{
    if (h.narrowed) return h.narrowed > 0 ? CCP_OK : CCP_ERR_UNSUPPORTED;
    hipStream_t s = v.stream;
    const long n0 = v.geom.ch_stride;
    long total = 0;
    h.fbase.assign((size_t)h.levels, 0);
    for (int k = 1; k < h.levels; ++k) {
        h.fbase[k] = total;
        total += (h.opC > 1 ? 3 : 6) * h.size[k];          // one operator per channel: the vectors alone (cfstore has d, we, ws)
    }
    CCP_TRY(h.fbad.alloc(1));
    CCP_HIP(hipMemsetAsync(h.fbad.p, 0, sizeof(unsigned), s));
    CCP_TRY(h.t0f.alloc((size_t)n0));
    CCP_HIP(hipMemsetAsync(h.t0f.p, 0, sizeof(float) * n0, s));
    if (total > 0) {
        CCP_TRY(h.fstore.alloc((size_t)total));
        CCP_HIP(hipMemsetAsync(h.fstore.p, 0, sizeof(float) * total, s));
    }
    if (h.opC > 1) {
        const long ftotal = 3 * h.cbase.back() / 4 + 3L * h.opC * h.size.back();
        CCP_TRY(h.cfstore.alloc((size_t)ftotal));
        CCP_HIP(hipMemsetAsync(h.cfstore.p, 0, sizeof(float) * ftotal, s));
        h.cflv.assign((size_t)h.opC, std::vector<MgsLevel>((size_t)h.levels, MgsLevel{}));
    }
    h.flv.assign((size_t)h.levels, MgsLevel{});
    if (h.weighted) CCP_TRY(h.w32.alloc((size_t)(3 * n0 * h.opC)));
    for (int ch = 0; ch < h.opC; ++ch)
        for (int k = 0; k < h.levels; ++k) {
            const MgLevel &l = h.opC > 1 ? h.clv[(size_t)ch][k] : h.lv[k];
            MgsLevel &f = h.opC > 1 ? h.cflv[(size_t)ch][k] : h.flv[k];
            f.W = l.W;
            f.H = l.H;
            f.pitch = l.pitch;
            f.mask = l.mask;
            f.g0 = l.g0;
            if (k) {
                f.d = h.fcoef(ch, k, 0);
                f.we = h.fcoef(ch, k, 1);
                f.ws = h.fcoef(ch, k, 2);
            } else if (h.weighted) {                                // the copy of the handle's d, we, ws planes
                float *w = h.w32.p + 3 * n0 * ch;
                f.d = w;
                f.we = w + n0;
                f.ws = w + 2 * n0;
            }
        }
    CCP_TRY(narrow_launch(v, h));
    unsigned bad = 0;
    CCP_HIP(hipMemcpyAsync(&bad, h.fbad.p, sizeof(bad), hipMemcpyDeviceToHost, s));
    CCP_HIP(hipStreamSynchronize(s));
    h.narrowed = bad ? -1 : 1;
    return bad ? CCP_ERR_UNSUPPORTED : CCP_OK;
}

template <int KIND, bool POST, typename B, typename Z>
void tile32(hipStream_t s, dim3 grid, const MgsLevel &f, const B *b, const float *t, Z *z, const MgsLevel &c, const float *ec, float cs, int nu,
            const CgState *st)
{
    hipLaunchKernelGGL((k_mgs_tile<KIND, POST, B, Z>), grid, dim3(kBlock), mgs_tile_lds(nu), s, f, b, t, z, c, ec, cs, nu, st);
}

// a level-0 pass: b is the PCG's fp64 r; Z = double where the pass writes the PCG's z
template <bool POST, typename Z>
void tile32_top(int kind, hipStream_t s, dim3 grid, const MgsLevel &f, const double *b, const float *t, Z *z, const MgsLevel &c, const float *ec,
                float cs, int nu, const CgState *st)
{
    with_kind(kind, [&](auto K) { tile32<decltype(K)::value, POST>(s, grid, f, b, t, z, c, ec, cs, nu, st); });
}

dim3 tiles32(const MgsLevel &f) { return dim3((unsigned)((f.W + kMgsTileW - 1) / kMgsTileW), (unsigned)((f.H + kMgsTileH - 1) / kMgsTileH)); }

// vcycle in float: z0 := (double) M32^-1 (float) b0, the launch structure of vcycle in fp64
int vcycle32(MgHierarchy &h, hipStream_t s, const double *b0, double *z0, int nu, const CgState *st, int ch)
{
    const std::vector<MgsLevel> &flv = h.flevels_of(ch);
    const float *none = nullptr;
    const float cs = (float)h.cs;
    const MgsLevel &l0 = flv[0];
    if (h.levels == 1) {
        tile32_top<false>(h.kind0, s, dim3(1), l0, b0, none, z0, l0, none, 2.0f, nu, st);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    auto T = [&](int k) -> float * { return k ? h.fvec(k, 2) : h.t0f.p; };
    for (int k = 0; k < h.tail; ++k) {
        const MgsLevel &f = flv[k], &c = flv[k + 1];
        const dim3 rgrid = cells_grid(c.W, c.H);
        if (k == 0) {
            tile32_top<false>(h.kind0, s, tiles32(f), f, b0, none, T(0), f, none, 2.0f, nu, st);
            with_kind(h.kind0, [&](auto K) {
                hipLaunchKernelGGL((k_mgs_restrict<decltype(K)::value, double>), rgrid, dim3(kBlock), 0, s, f, b0, T(0), c, h.fvec(1, 0), st);
            });
        } else {
            const float *b = h.fvec(k, 0);
            tile32<kMgCoarse, false>(s, tiles32(f), f, b, none, T(k), f, none, 2.0f, nu, st);
            hipLaunchKernelGGL((k_mgs_restrict<kMgCoarse, float>), rgrid, dim3(kBlock), 0, s, f, b, T(k), c, h.fvec(k + 1, 0), st);
        }
    }
    const MgsTail t = tail_of<MgsTail>(flv, h.tail);
    hipLaunchKernelGGL(k_mgs_tail, dim3(1), dim3(kBlock), 0, s, t, static_cast<const float *>(h.fvec(h.tail, 0)), h.fvec(h.tail, 1), cs, nu, st);
    for (int k = h.tail - 1; k >= 0; --k) {
        const MgsLevel &f = flv[k], &c = flv[k + 1];
        const float *ec = h.fvec(k + 1, 1);
        if (k == 0) tile32_top<true>(h.kind0, s, tiles32(f), f, b0, static_cast<const float *>(T(0)), z0, c, ec, cs, nu, st);
        else tile32<kMgCoarse, true>(s, tiles32(f), f, static_cast<const float *>(h.fvec(k, 0)), static_cast<const float *>(T(k)), h.fvec(k, 1), c, ec, cs, nu, st);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// z0 := M^-1 b0 on level 0 (one channel, with channel ch's operator where the handle has one per channel); every launch
// is a no-op once st->active is 0 (st may be null)
int vcycle(MgHierarchy &h, hipStream_t s, const double *b0, double *z0, int nu, const CgState *st, int ch = 0)
{
    if (h.precision == CCP_MG_PRECISION_F32) return vcycle32(h, s, b0, z0, nu, st, ch);
    if (h.levels == 1) {                                            // a 1x1 image
        pre(h.kind0, s, dim3(1), h.levels_of(ch)[0], b0, z0, nu, st);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    return whole_levels(h, s, 0, b0, z0, nu, st, ch);
}

// ---- CCP_MG_CHANNELS_BATCHED (ccp_grid_mgb.hpp) ----------------------------------------------------------------------
// The dynamic LDS a k_mgb_tile launch asks for: the one figure behind the launch, the limit below and
// ccp_debug_mgb_tile_lds.
int tile_b_lds(int kind, int nu) { return mgb_tile_lds(kind, nu); }

// The stored-operator kind passes the 64 KiB a kernel may take without asking; the others come within 256 B of it
// (65,280 B at nu = 4) and are given their size too.  Once per device and process.
int tile_lds_limit()
{
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    CCP_HIP(hipGetDevice(&dev));
    const unsigned long long bit = dev < 64 ? 1ull << dev : 0;
    if (raised.load() & bit) return CCP_OK;
    for (int kind : {kMgSolve, kMgMasked, kMgCoarse})
        CCP_TRY(with_kind(kind, [](auto K) -> int {
            constexpr int KIND = decltype(K)::value;
            const int bytes = tile_b_lds(KIND, 4);                        // the largest nu
            CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mgb_tile<KIND, false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mgb_tile<KIND, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            return CCP_OK;
        }));
    raised.fetch_or(bit);
    return CCP_OK;
}

// C of level 0's t and of every coarse level's b, z, t, once per hierarchy
int batched_levels(const GridMgView &v, MgHierarchy &h)
{
    if (h.bC == v.channels && h.bt0.p) return CCP_OK;
    const int C = v.channels;
    const long n0 = v.geom.ch_stride;
    CCP_TRY(tile_lds_limit());
    if (h.opC > 1) {                                                // one operator per channel: k_pco_* (ccp_grid_pco.hpp)
        CCP_TRY(pco_tile_lds_limit());
        std::vector<MgTail> tails;
        for (int ch = 0; ch < h.opC; ++ch) tails.push_back(tail_of<MgTail>(h.clv[(size_t)ch], h.tail));
        CCP_TRY(h.ctails.alloc(tails.size()));
        CCP_HIP(hipMemcpyAsync(h.ctails.p, tails.data(), sizeof(MgTail) * tails.size(), hipMemcpyHostToDevice, v.stream));
        CCP_HIP(hipStreamSynchronize(v.stream));                    // (tails goes out of scope)
    }
    long total = 0;
    h.bbase.assign((size_t)h.levels, 0);
    for (int k = 1; k < h.levels; ++k) {
        h.bbase[k] = total;
        total += 3 * C * h.size[k];
    }
    CCP_TRY(h.bt0.alloc((size_t)(C * n0)));
    CCP_HIP(hipMemsetAsync(h.bt0.p, 0, sizeof(double) * C * n0, v.stream));
    if (total > 0) {
        CCP_TRY(h.bstore.alloc((size_t)total));
        CCP_HIP(hipMemsetAsync(h.bstore.p, 0, sizeof(double) * total, v.stream));
    }
    h.bC = C;
    return CCP_OK;
}

void batched_release(MgHierarchy &h)
{
    h.bt0.release();
    h.bstore.release();
    h.ctails.release();
    h.bat.release();
    h.bC = 0;
}

template <bool POST>
void tile_b(int kind, hipStream_t s, dim3 grid, const MgLevel &f, const double *b, const double *t, double *z, long fs, const MgLevel &c,
            const double *ec, long es, double cs, int nu, int C, const CgState *st)
{
    with_kind(kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        hipLaunchKernelGGL((k_mgb_tile<KIND, POST>), grid, dim3(mgb_tile_threads(KIND)), tile_b_lds(KIND, nu), s, f, b, t, z, fs, c, ec, es, cs, nu, C, st);
    });
}

// z0 := M^-1 b0 for all C channels (n0 doubles apart in b0 and z0): the launches of vcycle in fp64, each serving
// all channels; st: CgState[C] or null
int vcycle_batched(MgHierarchy &h, hipStream_t s, int C, long n0, const double *b0, double *z0, int nu, const CgState *st)
{
    const double *none = nullptr;
    if (h.opC > 1) {                                                 // one operator per channel: the same launches, the channel on grid z
        const std::vector<MgLevel> &lv = h.clv[0];                   // channel 0's descriptors; channel ch's coefficients OS(k) ch further
        auto OS = [&](int k) -> long { return k ? 4 * h.size[k] : h.os0; };
        auto S = [&](int k) -> long { return k ? h.size[k] : n0; };
        auto B = [&](int k) -> const double * { return k ? h.barr(k, 0) : b0; };
        auto Z = [&](int k) -> double * { return k ? h.barr(k, 1) : z0; };
        auto T = [&](int k) -> double * { return k ? h.barr(k, 2) : h.bt0.p; };
        if (h.levels == 1) return pco_tile(s, false, dim3(1), C, lv[0], OS(0), b0, none, z0, n0, lv[0], none, 0, 2.0, nu, st);
        for (int k = 0; k < h.tail; ++k) {
            CCP_TRY(pco_tile(s, false, tiles(lv[k]), C, lv[k], OS(k), B(k), none, T(k), S(k), lv[k], none, 0, 2.0, nu, st));
            CCP_TRY(pco_restrict(s, C, lv[k], OS(k), B(k), T(k), S(k), lv[k + 1], h.barr(k + 1, 0), S(k + 1), st));
        }
        CCP_TRY(pco_tail(s, C, h.ctails.p, B(h.tail), Z(h.tail), S(h.tail), S(h.tail), h.cs, nu, st));
        for (int k = h.tail - 1; k >= 0; --k)
            CCP_TRY(pco_tile(s, true, tiles(lv[k]), C, lv[k], OS(k), B(k), T(k), Z(k), S(k), lv[k + 1], h.barr(k + 1, 1), S(k + 1), h.cs, nu, st));
        return CCP_OK;
    }
    if (h.levels == 1) {
        tile_b<false>(h.kind0, s, dim3(1), h.lv[0], b0, none, z0, n0, h.lv[0], none, 0, 2.0, nu, C, st);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    auto S = [&](int k) -> long { return k ? h.size[k] : n0; };      // the channel stride of level k's vectors
    auto B = [&](int k) -> const double * { return k ? h.barr(k, 0) : b0; };
    auto Z = [&](int k) -> double * { return k ? h.barr(k, 1) : z0; };
    auto T = [&](int k) -> double * { return k ? h.barr(k, 2) : h.bt0.p; };
    const unsigned groups = (unsigned)((C + kMgbGroup - 1) / kMgbGroup);
    for (int k = 0; k < h.tail; ++k) {
        const MgLevel &f = h.lv[k], &c = h.lv[k + 1];
        const int kind = level_kind(h, k);
        tile_b<false>(kind, s, tiles(f), f, B(k), none, T(k), S(k), f, none, 0, 2.0, nu, C, st);
        dim3 grid = cells_grid(c.W, c.H);
        grid.z = groups;
        with_kind(kind, [&](auto K) {
            hipLaunchKernelGGL((k_mgb_restrict<decltype(K)::value>), grid, dim3(kBlock), 0, s, f, B(k), static_cast<const double *>(T(k)), S(k), c, 0,
                               h.barr(k + 1, 0), S(k + 1), C, st);
        });
    }
    const MgTail t = tail_of<MgTail>(h.lv, h.tail);
    hipLaunchKernelGGL(k_mgb_tail, dim3((unsigned)C), dim3(kBlock), 0, s, t, B(h.tail), Z(h.tail), S(h.tail), S(h.tail), h.cs, nu, st);
    for (int k = h.tail - 1; k >= 0; --k)
        tile_b<true>(level_kind(h, k), s, tiles(h.lv[k]), h.lv[k], B(k), static_cast<const double *>(T(k)), Z(k), S(k), h.lv[k + 1],
                     static_cast<const double *>(h.barr(k + 1, 1)), S(k + 1), h.cs, nu, C, st);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// ---- the PCG loop ----------------------------------------------------------------------------------------------------
// One loop (pcg_loop) serves the three modes.  A mode is a "steps" object: the launches of every step of the recurrence,
// and no control flow of the loop.  The wide passes (init, dot, update, direction) only launch; the products, the
// V-cycle and the one-block steps that consume a sum (check, set_rlen, alpha, beta) return a status: on row blocks they
// exchange ghost rows and all-reduce.  The loop itself reads s, st (the device's CgState[C]) and p, z, len (p = z copies
// len doubles) from the object.

// The step calls of the recurrence, written once for the two forms of the loop below: the start-up steps, and `count`
// iterations (the launches of an iteration are no-ops once st says so).
template <typename Steps>
int pcg_start(const Steps &S)
{
    CCP_TRY(S.residual());                                               // r = A x
    S.init();                                                            // r = b - r; r'r
    CCP_TRY(S.check());
    CCP_TRY(S.precondition());                                           // z = M r
    S.dot();
    CCP_TRY(S.set_rlen());                                               // rlen = r'z
    CCP_TRY(S.start_direction());                                        // p = z
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

template <typename Steps>
int pcg_iterate(const Steps &S, int count)
{
    for (int k = 0; k < count; ++k) {
        CCP_TRY(S.product());                                            // Ap, p'Ap partials
        CCP_TRY(S.alpha());                                              // alpha = r'z / p'Ap
        S.update();
        CCP_TRY(S.check());
        CCP_TRY(S.precondition());
        S.dot();
        CCP_TRY(S.beta());
        S.direction();                                                   // p = z + beta p
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// The enqueue-only form (ccp_grid_mg_conjugate_gradient_enqueue): S.st has been initialised on the device (k_mge_init);
// the start-up steps, exactly max_iteration iterations and the mode's finish go onto the stream, and nothing comes back.
template <typename Steps>
int pcg_enqueue(const Steps &S, int max_iteration)
{
    CCP_TRY(pcg_start(S));
    CCP_TRY(pcg_iterate(S, max_iteration));
    return S.finish();
}

// The synchronous form: the states go up from the host, and come back after the start-up steps, after every batch of 16
// iterations (the loop stops issuing once no channel is active) and at the end.
// host: C states of the caller's (the read-backs land there); report: C entries or null.  `seconds` is the time of this
// call in every entry: one channel's solve, or in batched mode the whole solve.
template <typename Steps>
int pcg_loop(const Steps &S, MgHierarchy &h, CgState *host, int C, int max_iteration, ccp_gs_report *report)
{
    hipStream_t s = S.s;
    const size_t st_bytes = sizeof(CgState) * (size_t)C;
    auto read_back = [&]() -> int {
        CCP_HIP(hipMemcpyAsync(host, S.st, st_bytes, hipMemcpyDeviceToHost, s));
        CCP_HIP(hipStreamSynchronize(s));
        return CCP_OK;
    };
    auto any_active = [&]() {
        for (int c = 0; c < C; ++c)
            if (host[c].active) return true;
        return false;
    };
    for (int c = 0; c < C; ++c) {
        host[c] = CgState{};
        host[c].active = 1;
    }
    CCP_HIP(hipMemcpyAsync(S.st, host, st_bytes, hipMemcpyHostToDevice, s));
    CCP_HIP(hipEventRecord(h.ev0, s));
    CCP_TRY(pcg_start(S));
    CCP_TRY(read_back());
    int issued = 0;
    bool active = any_active() && max_iteration > 0;
    while (active && issued < max_iteration) {
        const int batch = std::min(16, max_iteration - issued);
        CCP_TRY(pcg_iterate(S, batch));
        issued += batch;
        CCP_TRY(read_back());
        active = any_active();
    }
    CCP_TRY(S.finish());                                                 // (nothing, but in CCP_MG_NULLSPACE_CONSTANT mode)
    CCP_HIP(hipEventRecord(h.ev1, s));
    CCP_TRY(read_back());
    if (report) {
        float ms = 0.f;
        CCP_HIP(hipEventElapsedTime(&ms, h.ev0, h.ev1));
        for (int c = 0; c < C; ++c) {
            report[c].iterations = host[c].iterations;
            report[c].converged = host[c].converged;
            report[c].last_l1_step = host[c].r1norm;
            report[c].seconds = ms * 1e-3;
        }
    }
    return CCP_OK;
}

// What the steps of every mode work on
struct PcgArgs {
    MgHierarchy *h;
    hipStream_t s;
    dim3 agrid;                      // of the product
    int apply_blocks, blocks;        // the partial sums (per channel) a product / a wide pass leaves
    long n, len, ps;                 // doubles of a channel, of p = z, of a channel's partial sums
    double epsilon;
    int nu;
    const double *b;
    double *x, *r, *z, *p, *ap, *part;
    CgState *st;
    // The stop test relative to |b| (ccp_grid_mgr.hpp; eps null: the absolute one, against `epsilon`): the device words of
    // the channel's threshold and norm (batched: of channel 0, the others follow), the partial sums of b'b laid out as
    // `part`, and what the threshold step reads beside `epsilon` -- epsilon_rel and the operator's status word (or null)
    double *eps = nullptr, *bnorm = nullptr, *bpart = nullptr;
    double epsilon_rel = 0.0;
    const unsigned *status = nullptr;
    // rows folded so that the product's grid has ~2,048 blocks per channel group (and as many partial sums for alpha)
    void shape(int W, int rows, long count, unsigned groups = 1)
    {
        const unsigned agx = cells_grid((W + 1) / 2, 1).x;
        agrid = dim3(agx, (unsigned)std::max(1, std::min(rows, (int)(1024 / agx))), 2 * groups);
        apply_blocks = (int)(agrid.x * agrid.y * 2);
        blocks = (int)std::max<long>(1, std::min<long>(2048, (count + kBlock - 1) / kBlock));
        n = len = count;
    }
    void bind(PcgWork &w, long off)   // the vectors from `off` on
    {
        r = w.r.p + off, z = w.z.p + off, p = w.p.p + off, ap = w.ap.p + off;
        part = w.partial.p, ps = w.ps, st = w.state.p;
    }
    // the first direction, p = z, and what a mode still owes x when the loop ends
    int start_direction() const
    {
        CCP_HIP(hipMemcpyAsync(p, z, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
        return CCP_OK;
    }
    int finish() const { return CCP_OK; }
};

// One channel of a one-block handle: k_cg_* / k_mg_*.  The caller sets b and x per channel.
struct ChannelSteps : PcgArgs {
    int ch = 0;                      // whose operator (one operator per channel; 0 otherwise)
    int apply(const double *in, double *out, bool dot) const              // the product of an iteration stops with the loop
    {
        const CgState *a = dot ? st : nullptr;
        with_kind(h->kind0, [&](auto K) {
            with_bool(dot, [&](auto D) {
                hipLaunchKernelGGL((k_mg_apply<decltype(K)::value, decltype(D)::value>), agrid, dim3(kBlock), 0, s, h->levels_of(ch)[0], in, out, part, a);
            });
        });
        return CCP_OK;
    }
    int residual() const { return apply(x, r, false); }
    int product() const { return apply(p, ap, true); }
    int precondition() const { return vcycle(*h, s, r, z, nu, st, ch); }
    // the relative stop test's one-block step after its init pass: bnorm and eps from the partial sums of b'b
    void threshold() const
    {
        hipLaunchKernelGGL(k_mgr_threshold, dim3(1), dim3(kBlock), 0, s, static_cast<const double *>(bpart), blocks, epsilon, epsilon_rel, status,
                           bnorm, eps);
    }
    void init() const
    {
        if (!eps) {
            hipLaunchKernelGGL(k_cg_init, dim3(blocks), dim3(kBlock), 0, s, b, r, p, n, part);
            return;
        }
        hipLaunchKernelGGL(k_mgr_init, dim3(blocks), dim3(kBlock), 0, s, b, r, p, n, part, bpart);
        threshold();
    }
    void dot() const { hipLaunchKernelGGL(k_cg_dot, dim3(blocks), dim3(kBlock), 0, s, r, z, n, part, st); }
    void update() const { hipLaunchKernelGGL(k_cg_update, dim3(blocks), dim3(kBlock), 0, s, x, p, r, ap, n, part, st); }
    void direction() const { hipLaunchKernelGGL(k_cg_direction, dim3(blocks), dim3(kBlock), 0, s, p, z, n, st); }
    // the one-block steps read `count` sums at `sum`
    int check(const double *sum, int count) const
    {
        if (eps) hipLaunchKernelGGL(k_mgr_check, dim3(1), dim3(kBlock), 0, s, sum, count, static_cast<const double *>(eps), st);
        else hipLaunchKernelGGL(k_mg_check, dim3(1), dim3(kBlock), 0, s, sum, count, epsilon, st);
        return CCP_OK;
    }
    int set_rlen(const double *sum, int count) const { hipLaunchKernelGGL(k_cg_set_rlen, dim3(1), dim3(kBlock), 0, s, sum, count, st); return CCP_OK; }
    int alpha(const double *sum, int count) const { hipLaunchKernelGGL(k_cg_alpha, dim3(1), dim3(kBlock), 0, s, sum, count, st); return CCP_OK; }
    int beta(const double *sum, int count) const { hipLaunchKernelGGL(k_mg_beta, dim3(1), dim3(kBlock), 0, s, sum, count, st); return CCP_OK; }
    int check() const { return check(part, blocks); }
    int set_rlen() const { return set_rlen(part, blocks); }
    int alpha() const { return alpha(part, apply_blocks); }
    int beta() const { return beta(part, blocks); }
};

// One channel of a weighted handle in CCP_MG_NULLSPACE_CONSTANT mode (ccp_grid_mgn.hpp; the loop: include/ccp_gs.h): the
// product, the V-cycle, the update and the checks are ChannelSteps'; the sums carry sum(z) and sum(r) along and the
// directions subtract mean(z).
struct NullspaceSteps : ChannelSteps {
    MgnLay lay;
    double pixels;                   // W H
    MgnState *ns;
    double *npart;                   // 3 x `blocks` partial sums
    const unsigned *hold = nullptr;  // the enqueue solve: the operator's status word (k_mgn_means)
    void means(const double *a, const double *b2, int which) const
    {
        hipLaunchKernelGGL(k_mgn_sums, dim3(blocks), dim3(kBlock), 0, s, a, b2, lay, npart);
        hipLaunchKernelGGL(k_mgn_means, dim3(1), dim3(kBlock), 0, s, static_cast<const double *>(npart), blocks, pixels, which, ns, hold);
    }
    void shift() const { hipLaunchKernelGGL(k_mgn_shift, dim3(blocks), dim3(kBlock), 0, s, x, lay, static_cast<const MgnState *>(ns)); }
    int residual() const                                                 // bm, m0; r = A x
    {
        means(b, x, kMgnStart);
        return apply(x, r, false);
    }
    void init() const
    {
        if (!eps) {
            hipLaunchKernelGGL(k_mgn_init, dim3(blocks), dim3(kBlock), 0, s, b, r, lay, static_cast<const MgnState *>(ns), part);
            return;
        }
        hipLaunchKernelGGL(k_mgr_init_constant, dim3(blocks), dim3(kBlock), 0, s, b, r, lay, static_cast<const MgnState *>(ns), part, bpart);
        threshold();
    }
    void dot() const { hipLaunchKernelGGL(k_mgn_dot, dim3(blocks), dim3(kBlock), 0, s, r, z, n, npart, st); }
    int set_rlen() const { hipLaunchKernelGGL(k_mgn_rz<true>, dim3(1), dim3(kBlock), 0, s, static_cast<const double *>(npart), blocks, pixels, st, ns); return CCP_OK; }
    int beta() const { hipLaunchKernelGGL(k_mgn_rz<false>, dim3(1), dim3(kBlock), 0, s, static_cast<const double *>(npart), blocks, pixels, st, ns); return CCP_OK; }
    void direction() const { hipLaunchKernelGGL(k_mgn_direction<false>, dim3(blocks), dim3(kBlock), 0, s, p, z, lay, st, static_cast<const MgnState *>(ns)); }
    int start_direction() const
    {
        hipLaunchKernelGGL(k_mgn_direction<true>, dim3(blocks), dim3(kBlock), 0, s, p, z, lay, st, static_cast<const MgnState *>(ns));
        return CCP_OK;
    }
    int finish() const                                                   // x += m0 - mean(x); the mean it then has
    {
        means(x, nullptr, kMgnClose);
        shift();
        means(x, nullptr, kMgnReport);
        return CCP_OK;
    }
};

// All C channels of a one-block handle (n doubles apart in every vector): the sequential launches, each for all channels
struct BatchedSteps : PcgArgs {
    int C;
    dim3 vgrid, sgrid;               // of a wide pass, of a one-block step (a block per channel)
    int apply(const double *in, double *out, bool dot) const
    {
        const CgState *a = dot ? st : nullptr;
        if (h->opC > 1) return pco_apply(s, dot, agrid, C, h->clv[0][0], h->os0, in, out, n, part, ps, a);
        with_kind(h->kind0, [&](auto K) {
            with_bool(dot, [&](auto D) {
                hipLaunchKernelGGL((k_mgb_apply<decltype(K)::value, decltype(D)::value>), agrid, dim3(kBlock), 0, s, h->lv[0], in, out, n, part, ps, C, a);
            });
        });
        return CCP_OK;
    }
    int residual() const { return apply(x, r, false); }
    int product() const { return apply(p, ap, true); }
    int precondition() const { return vcycle_batched(*h, s, C, n, r, z, nu, st); }
    void init() const
    {
        if (!eps) {
            hipLaunchKernelGGL(k_mgb_init, vgrid, dim3(kBlock), 0, s, b, r, p, n, part, ps);
            return;
        }
        hipLaunchKernelGGL(k_mgr_init_batched, vgrid, dim3(kBlock), 0, s, b, r, p, n, part, bpart, ps);
        hipLaunchKernelGGL(k_mgr_threshold_batched, sgrid, dim3(kBlock), 0, s, static_cast<const double *>(bpart), ps, blocks, epsilon, epsilon_rel,
                           status, bnorm, eps);
    }
    void dot() const { hipLaunchKernelGGL(k_mgb_dot, vgrid, dim3(kBlock), 0, s, r, z, n, part, ps, st); }
    void update() const { hipLaunchKernelGGL(k_mgb_update, vgrid, dim3(kBlock), 0, s, x, p, r, ap, n, part, ps, st); }
    void direction() const { hipLaunchKernelGGL(k_mgb_direction, vgrid, dim3(kBlock), 0, s, p, z, n, st); }
    int check() const
    {
        if (eps) hipLaunchKernelGGL(k_mgr_check_batched, sgrid, dim3(kBlock), 0, s, part, ps, blocks, static_cast<const double *>(eps), st);
        else hipLaunchKernelGGL(k_mgb_check, sgrid, dim3(kBlock), 0, s, part, ps, blocks, epsilon, st);
        return CCP_OK;
    }
    int set_rlen() const { hipLaunchKernelGGL(k_mgb_set_rlen, sgrid, dim3(kBlock), 0, s, part, ps, blocks, st); return CCP_OK; }
    int alpha() const { hipLaunchKernelGGL(k_mgb_alpha, sgrid, dim3(kBlock), 0, s, part, ps, apply_blocks, st); return CCP_OK; }
    int beta() const { hipLaunchKernelGGL(k_mgb_beta, sgrid, dim3(kBlock), 0, s, part, ps, blocks, st); return CCP_OK; }
};

// The relative stop test of one enqueue solve (ccp_grid_mg_conjugate_gradient_enqueue_relative): epsilon_rel and where in
// h.erel the thresholds, the norms and the partial sums of b'b live.  `epsilon` of the solve is epsilon_abs then.
struct PcgRelative {
    double epsilon_rel;
    double *eps, *bnorm, *bpart;
    const unsigned *status;
    // into a steps object: channel ch's words (batched: ch = 0)
    void bind(PcgArgs &a, int ch) const
    {
        a.eps = eps + ch, a.bnorm = bnorm + ch, a.bpart = bpart;
        a.epsilon_rel = epsilon_rel, a.status = status;
    }
};

// ccp_grid_mg_conjugate_gradient in batched mode, on the levels and the work set pcg_ready made.  enqueue: the host-free
// form, on the states at h.estate; rel: its relative stop test, or null
int pcg_batched(const GridMgView &v, MgHierarchy &h, double epsilon, int max_iteration, int nu, ccp_gs_report *report, bool enqueue,
                const PcgRelative *rel)
{
    const int C = v.channels;
    const unsigned groups = (unsigned)((C + kMgbGroup - 1) / kMgbGroup);
    BatchedSteps S{};
    S.h = &h, S.s = v.stream, S.C = C, S.epsilon = epsilon, S.nu = nu;
    S.shape(v.geom.W, v.geom.H, v.geom.ch_stride, groups);               // (the sequential loop's grids within a channel)
    S.len = C * S.n;
    S.vgrid = dim3((unsigned)S.blocks, (unsigned)C);
    S.sgrid = dim3((unsigned)C);
    S.bind(h.bat, 0);
    S.b = v.b, S.x = v.x;
    if (enqueue) {
        S.st = h.estate.p;
        if (rel) rel->bind(S, 0);
        return pcg_enqueue(S, max_iteration);
    }
    std::vector<CgState> host((size_t)C);
    return pcg_loop(S, h, host.data(), C, max_iteration, report);
}

// ---- row blocks ----------------------------------------------------------------------------------------------------
constexpr int kMgGhost = 8;          // ghost rows per neighbour side of a distributed level: 2 x the largest nu

struct Net {
    const RcclApi *api;
    ccp_comm *comm;
    int rank, world;
    hipStream_t s;
};

// Rows of the distributed level k to the neighbours' ghost rows next to their owned rows, theirs into ours: up to `req`
// rows per side (fewer when the sending block owns fewer), `elem` bytes per value of type t, one RCCL group.
int exchange_rows(const MgHierarchy &h, const Net &n, int k, void *base, size_t elem, ncclDataType_t t, int req)
{
    if (n.world == 1) return CCP_OK;
    const MgLevel &l = h.lv[k];
    const std::vector<int> &o = h.own[k];
    const size_t row = (size_t)2 * l.pitch;            // values per row
    char *p = static_cast<char *>(base);
    auto at = [&](int r) { return p + (size_t)r * row * elem; };
    const int mine = o[n.rank + 1] - o[n.rank];
    const int snd = std::min(req, mine);
    CCP_RCCL(n.api->GroupStart());
    ncclResult_t r = ncclSuccess;
    if (n.rank > 0) {
        const int rcv = std::min(req, o[n.rank] - o[n.rank - 1]);
        r = n.api->Send(at(l.lo), (size_t)snd * row, t, n.rank - 1, n.comm->comm, n.s);
        if (r == ncclSuccess) r = n.api->Recv(at(l.lo - rcv), (size_t)rcv * row, t, n.rank - 1, n.comm->comm, n.s);
    }
    if (n.rank + 1 < n.world && r == ncclSuccess) {
        const int rcv = std::min(req, o[n.rank + 2] - o[n.rank + 1]);
        r = n.api->Send(at(l.hi - snd), (size_t)snd * row, t, n.rank + 1, n.comm->comm, n.s);
        if (r == ncclSuccess) r = n.api->Recv(at(l.hi), (size_t)rcv * row, t, n.rank + 1, n.comm->comm, n.s);
    }
    const ncclResult_t e = n.api->GroupEnd();
    if (r != ncclSuccess) return rccl_fail(r, "ncclSend/ncclRecv", __FILE__, __LINE__);
    CCP_RCCL(e);
    return CCP_OK;
}

int exchange_rows(const MgHierarchy &h, const Net &n, int k, double *base, int req)
{
    return exchange_rows(h, n, k, base, sizeof(double), ncclDouble, req);
}

// The one-block hierarchy over the partition `part` (world + 1 global rows).  Level k+1 stays distributed while every
// block boundary of level k is even, every block owns >= kMgGhost rows of level k+1 and level k+1 is above the tail.
// Every rank takes the same decisions from the same partition.  COLLECTIVE (ghost rows of the coefficients, the sums
// that form the first whole level).
int build_rowblocked(const GridMgView &v, const Net &n, MgHierarchy **out)
{
    MgHierarchy *h = new MgHierarchy();
    std::unique_ptr<MgHierarchy> own(h);
    h->rowblocked = true;
    h->kind0 = v.masked ? kMgMasked : kMgSolve;
    std::vector<int> Ws{v.geom.W}, Hs{v.geom.H};
    while (Ws.back() > 1 || Hs.back() > 1) {
        Ws.push_back((Ws.back() + 1) / 2);
        Hs.push_back((Hs.back() + 1) / 2);
    }
    h->levels = (int)Ws.size();
    h->tail = h->levels;
    for (int k = 1; k < h->levels; ++k)
        if (Ws[k] <= kMgTailSide && Hs[k] <= kMgTailSide) {
            h->tail = k;
            break;
        }
    if (h->levels - h->tail > kMgTailLevels) return CCP_ERR_STATE;
    h->own.emplace_back(v.part, v.part + n.world + 1);
    h->dist = 1;
    for (int k = 0; k + 1 < h->tail; ++k) {
        const std::vector<int> &o = h->own[k];
        std::vector<int> next(o.size());
        bool ok = true;
        for (int r = 1; r < n.world; ++r) {
            ok = ok && o[r] % 2 == 0;
            next[r] = o[r] / 2;
        }
        next[n.world] = Hs[k + 1];
        for (int r = 0; r < n.world; ++r) ok = ok && next[r + 1] - next[r] >= kMgGhost;
        if (!ok) break;
        h->own.push_back(next);
        h->dist = k + 2;
    }
    long total = 0;
    for (int k = 0; k < h->levels; ++k) {
        MgLevel l{};
        l.W = Ws[k];
        l.pitch = k ? (((long)l.W + 1) / 2 + 15) / 16 * 16 : v.geom.pitch;
        if (k < h->dist) {
            const int ob = h->own[k][n.rank], oe = h->own[k][n.rank + 1];
            // (the top ghost zone keeps local row 0 on an even global row: local parity is global parity)
            const int gt = n.rank > 0 ? std::min(ob, kMgGhost + (ob & 1)) : 0;
            const int gb = n.rank + 1 < n.world ? std::min(kMgGhost, Hs[k] - oe) : 0;
            l.y0 = ob - gt;
            l.lo = gt;
            l.hi = gt + (oe - ob);
            l.H = l.hi + gb;
        } else {
            l.H = l.hi = Hs[k];
        }
        h->lv.push_back(l);
        h->base.push_back(k ? total : 0);
        h->size.push_back(k ? (long)l.H * 2 * l.pitch : 0);
        total += 6 * h->size.back();
    }
    MgLevel &l0 = h->lv[0];
    l0.g0 = v.geom;
    l0.g0.y0 = l0.y0;
    l0.g0.local_rows = l0.H;
    l0.g0.own_lo = l0.lo;
    l0.g0.own_hi = l0.hi;
    l0.g0.ch_stride = (long)l0.H * 2 * l0.pitch;
    const long n0 = l0.g0.ch_stride, row = 2 * l0.pitch;
    CCP_TRY(h->t0.alloc((size_t)n0));
    CCP_HIP(hipMemsetAsync(h->t0.p, 0, sizeof(double) * n0, n.s));
    if (total > 0) {
        CCP_TRY(h->store.alloc((size_t)total));
        CCP_HIP(hipMemsetAsync(h->store.p, 0, sizeof(double) * total, n.s));
    }
    if (v.masked) {
        CCP_TRY(h->mask0.alloc((size_t)n0));
        CCP_HIP(hipMemsetAsync(h->mask0.p, 0, (size_t)n0, n.s));
        CCP_HIP(hipMemcpyAsync(h->mask0.p + l0.lo * row, v.mask + (long)v.geom.own_lo * row, (size_t)((l0.hi - l0.lo) * row),
                               hipMemcpyDeviceToDevice, n.s));
        CCP_TRY(exchange_rows(*h, n, 0, h->mask0.p, 1, ncclUint8, kMgGhost));
        l0.mask = h->mask0.p;
    }
    for (int k = 1; k < h->levels; ++k) {
        h->lv[k].d = h->arr(k, 0);
        h->lv[k].we = h->arr(k, 1);
        h->lv[k].ws = h->arr(k, 2);
    }
    for (int k = 0; k + 1 < h->levels; ++k) {
        const int c = k + 1;
        double *d = h->arr(c, 0), *we = h->arr(c, 1), *ws = h->arr(c, 2);
        const MgLevel &f = h->lv[k], &cl = h->lv[c];
        if (c < h->dist) {                               // the owned coarse rows, then their ghost rows
            coarsen(level_kind(*h, k), n.s, f, cl, cl.lo, cl.hi - cl.lo, d, we, ws);
            CCP_HIP(hipGetLastError());
            for (double *a : {d, we, ws}) CCP_TRY(exchange_rows(*h, n, c, a, kMgGhost));
        } else if (c == h->dist) {                       // every rank's share of the first whole level, summed (exact)
            const int fb = f.y0 + f.lo, fe = f.y0 + f.hi;
            coarsen(level_kind(*h, k), n.s, f, cl, fb / 2, (fe + 1) / 2 - fb / 2, d, we, ws);
            CCP_HIP(hipGetLastError());
            CCP_RCCL(n.api->AllReduce(d, d, (size_t)(3 * h->size[c]), ncclDouble, ncclSum, n.comm->comm, n.s));
        } else {
            coarsen(kMgCoarse, n.s, f, cl, 0, cl.H, d, we, ws);
            CCP_HIP(hipGetLastError());
        }
    }
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return CCP_ERR_HIP;
    *out = own.release();
    return CCP_OK;
}

int hierarchy_rowblocked(const GridMgView &v, const Net &n, MgHierarchy **out)
{
    if (*v.cache && !(*v.cache)->rowblocked) mg_release(v.cache);
    if (!*v.cache) CCP_TRY(build_rowblocked(v, n, v.cache));
    *out = *v.cache;
    return CCP_OK;
}

// z0 := M^-1 b0 on level 0's owned rows (one channel; b0 and z0 in level 0's layout, b0's owned rows current).  The
// distributed levels exchange their right-hand side (2 nu rows) before pre-smoothing, the pre-smoothed t (2 nu rows)
// after it and the coarse correction (nu + 1 rows) before post-smoothing; the first whole level is every rank's
// restriction of its own rows, summed.  COLLECTIVE: every rank issues the same messages whatever st says.
int vcycle_rowblocked(MgHierarchy &h, const Net &n, const double *b0, double *z0, int nu, const CgState *st)
{
    if (h.levels == 1) return vcycle(h, n.s, b0, z0, nu, st);       // (nothing to exchange)
    auto B = [&](int k) -> double * { return k ? h.arr(k, 3) : const_cast<double *>(b0); };
    auto Z = [&](int k) -> double * { return k ? h.arr(k, 4) : z0; };
    auto T = [&](int k) -> double * { return k ? h.arr(k, 5) : h.t0.p; };
    for (int k = 0; k < h.dist; ++k) {
        const MgLevel &f = h.lv[k], &c = h.lv[k + 1];
        CCP_TRY(exchange_rows(h, n, k, B(k), 2 * nu));
        pre(level_kind(h, k), n.s, tiles(f), f, B(k), T(k), nu, st);
        CCP_TRY(exchange_rows(h, n, k, T(k), 2 * nu));
        if (k + 1 < h.dist) {
            restrict_rows(level_kind(h, k), n.s, f, B(k), T(k), c, c.lo, c.hi - c.lo, B(k + 1), st);
        } else {
            const int fb = f.y0 + f.lo, fe = f.y0 + f.hi;
            CCP_HIP(hipMemsetAsync(B(k + 1), 0, sizeof(double) * h.size[k + 1], n.s));
            restrict_rows(level_kind(h, k), n.s, f, B(k), T(k), c, fb / 2, (fe + 1) / 2 - fb / 2, B(k + 1), st);
            CCP_HIP(hipGetLastError());
            CCP_RCCL(n.api->AllReduce(B(k + 1), B(k + 1), (size_t)h.size[k + 1], ncclDouble, ncclSum, n.comm->comm, n.s));
        }
        CCP_HIP(hipGetLastError());
    }
    CCP_TRY(whole_levels(h, n.s, h.dist, b0, z0, nu, st));
    for (int k = h.dist - 1; k >= 0; --k) {
        if (k + 1 < h.dist) CCP_TRY(exchange_rows(h, n, k + 1, Z(k + 1), nu + 1));
        post(level_kind(h, k), n.s, h.lv[k], B(k), T(k), Z(k), h.lv[k + 1], Z(k + 1), 2.0, nu, st);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// One channel of a row block, on the owned rows (r, z, p, ap point at them): a product fetches one ghost row of its
// input first, and every partial sum is reduced to one double and all-reduced before the one-block step that consumes
// it, so every rank takes the same decisions.  COLLECTIVE: every rank issues the same messages whatever st says.
struct RowSteps : ChannelSteps {
    const Net *net;
    double *total;                   // the communicator's scratch: the sum over every rank
    int sums(int count) const
    {
        hipLaunchKernelGGL(k_reduce_to_one, dim3(1), dim3(kBlock), 0, s, part, (long)count, total);
        CCP_HIP(hipGetLastError());
        CCP_RCCL(net->api->AllReduce(total, total, 1, ncclDouble, ncclSum, net->comm->comm, s));
        return CCP_OK;
    }
    int apply(double *in, double *out, bool dot) const                    // in, out: whole vectors of level 0
    {
        CCP_TRY(exchange_rows(*h, *net, 0, in, 1));
        ChannelSteps::apply(in, out, dot);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    int residual() const
    {
        CCP_HIP(hipMemcpyAsync(p, x, sizeof(double) * n, hipMemcpyDeviceToDevice, s));   // x with ghost rows, in p
        return apply(h->seq.p.p, h->seq.r.p, false);
    }
    int product() const { return apply(h->seq.p.p, h->seq.ap.p, true); }
    int precondition() const { return vcycle_rowblocked(*h, *net, h->seq.r.p, h->seq.z.p, nu, st); }
    int check() const { CCP_TRY(sums(blocks)); return ChannelSteps::check(total, 1); }
    int set_rlen() const { CCP_TRY(sums(blocks)); return ChannelSteps::set_rlen(total, 1); }
    int alpha() const { CCP_TRY(sums(apply_blocks)); return ChannelSteps::alpha(total, 1); }
    int beta() const { CCP_TRY(sums(blocks)); return ChannelSteps::beta(total, 1); }
};

// The checks every rank makes alike, before any collective call, then the hierarchy (collective on its first use)
int prepare_rowblocked(ccp_grid *g, int32_t smoothing_sweeps, bool need_nu, GridMgView *v, Net *n, int *nu, MgHierarchy **h)
{
    CCP_TRY(grid_mg_view(g, v));
    if (v->weighted) return CCP_ERR_UNSUPPORTED;                   // weighted handles are single blocks
    if (v->cfg.precision != CCP_MG_PRECISION_F64) return CCP_ERR_UNSUPPORTED;   // the fp32 V-cycle too (a world-1 communicator on a whole image)
    if (v->cfg.channels != CCP_MG_CHANNELS_SEQUENTIAL) return CCP_ERR_UNSUPPORTED;   // ... and the batched mode
    if (v->cfg.smoother != CCP_MG_SMOOTHER_POINT) return CCP_ERR_UNSUPPORTED;   // ... and the line smoother
    if (!v->comm) return CCP_ERR_STATE;
    n->api = rccl_api();
    if (!n->api) return CCP_ERR_RCCL;
    n->comm = v->comm;
    n->rank = v->comm->rank;
    n->world = v->comm->world;
    n->s = v->stream;
    if (n->world > 1 && v->ghost < 1) return CCP_ERR_STATE;
    if (need_nu) {
        CCP_TRY(sweeps_arg(smoothing_sweeps, nu));
        for (int r = 0; r < n->world; ++r)
            if (v->part[r + 1] - v->part[r] < 2 * *nu) return CCP_ERR_UNSUPPORTED;
    }
    return hierarchy_rowblocked(*v, *n, h);
}

int check_handle(ccp_grid *g, GridMgView *v)
{
    CCP_TRY(grid_mg_view(g, v));
    if (!v->one_block) return CCP_ERR_STATE;
    if (v->weighted && !v->wd) return CCP_ERR_STATE;              // no operator set (or the last one was refused)
    return CCP_OK;
}

// ---- CCP_MG_NULLSPACE_CONSTANT (ccp_grid_mgn.hpp) ----------------------------------------------------------------------
// (only a weighted handle can hold the value: kOptions)
bool constant_mode(const GridMgView &v) { return v.cfg.nullspace == CCP_MG_NULLSPACE_CONSTANT; }

// The census of the handle's operators into h.nscount, one word per operator, which the caller has cleared (nullspace_ready
// by a memset, the refresh in k_mge_clear): one launch
int census_launch(const GridMgView &v, MgHierarchy &h)
{
    dim3 grid = cells_grid(v.geom.W, v.geom.H);
    grid.z = (unsigned)v.op_channels;
    hipLaunchKernelGGL(k_mgn_census, grid, dim3(kBlock), 0, v.stream, v.wd, v.op_stride, (long)v.geom.ch_stride, v.geom.W, v.geom.H,
                       (long)v.geom.pitch, h.nscount.p);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// The mode's buffers, once per hierarchy, and the census of the handle's operators, once per installed operator (one
// read-back): CCP_ERR_UNSUPPORTED unless every one is floating
int nullspace_ready(const GridMgView &v, MgHierarchy &h)
{
    if (!constant_mode(v)) return CCP_OK;
    if (!h.nspart.p) {
        CCP_TRY(h.nscount.alloc((size_t)kMaxChannels));
        CCP_TRY(h.nsstate.alloc((size_t)kMaxChannels));
        CCP_TRY(h.nspart.alloc((size_t)(3 * 2048)));
    }
    MgNullspace &ns = *v.ns;
    if (ns.floating < 0) {
        const int sets = v.op_channels;
        unsigned bad[kMaxChannels] = {};
        CCP_HIP(hipMemsetAsync(h.nscount.p, 0, sizeof(unsigned) * kMaxChannels, v.stream));
        CCP_TRY(census_launch(v, h));
        CCP_HIP(hipMemcpyAsync(bad, h.nscount.p, sizeof(unsigned) * (size_t)sets, hipMemcpyDeviceToHost, v.stream));
        CCP_HIP(hipStreamSynchronize(v.stream));
        ns.floating = 1;
        for (int k = 0; k < sets; ++k)
            if (bad[k]) ns.floating = 0;
    }
    return ns.floating ? CCP_OK : CCP_ERR_UNSUPPORTED;
}

MgnLay nullspace_layout(const GridMgView &v) { return MgnLay{v.geom.W, 2 * v.geom.H, (int)v.geom.pitch}; }

// ---- one solve, three entry points -------------------------------------------------------------------------------------
// ccp_grid_mg_conjugate_gradient is pcg_ready then pcg_solve; ccp_grid_mg_prepare is pcg_ready alone, and
// ccp_grid_mg_conjugate_gradient_enqueue is pcg_solve alone in its enqueue form (enqueue_solve; _enqueue_relative is the
// same with the stop test of ccp_grid_mgr.hpp).

// The combinations of options that the one-block calls refuse, before anything is built (the row-block calls:
// prepare_rowblocked).  The line smoother serves a weighted handle, the fp64 V-cycle and the sequential channel mode;
// the constant null space the sequential channel mode.
int config_check(const GridMgView &v)
{
    const MgConfig &c = v.cfg;
    const bool sequential = c.channels == CCP_MG_CHANNELS_SEQUENTIAL, line = c.smoother == CCP_MG_SMOOTHER_LINE;
    if (!sequential && c.precision == CCP_MG_PRECISION_F32) return CCP_ERR_UNSUPPORTED;
    if (line && (!v.weighted || c.precision != CCP_MG_PRECISION_F64 || !sequential)) return CCP_ERR_UNSUPPORTED;
    if (!constant_mode(v)) return CCP_OK;
    if (!sequential) return CCP_ERR_UNSUPPORTED;
    // A line-smoothed level of one row or one column: its one line along that direction has no neighbour across and no
    // lambda (the coarse operators of a floating operator are floating too), so the exact line solve would be a solve of
    // the singular operator itself.  Lines run on level 0 and on every coarse level above the tail, the levels with a side
    // > kMgTailSide (build): 33x1 at level 0, 129x2 at its level 1 (65x1), 2048x32 at its level 5 (64x1).
    if (line)
        for (int k = 0, W = v.geom.W, H = v.geom.H; k == 0 || W > kMgTailSide || H > kMgTailSide; ++k, W = (W + 1) / 2, H = (H + 1) / 2)
            if (W == 1 || H == 1) return CCP_ERR_UNSUPPORTED;
    return CCP_OK;
}

// Everything a V-cycle in the view's configuration needs that allocates or reads back.  Every step is a no-op once it is done.
int vcycle_ready(const GridMgView &v, MgHierarchy **out)
{
    MgHierarchy *h = nullptr;
    CCP_TRY(hierarchy(v, &h));
    CCP_TRY(line_planes(v, *h));
    if (v.cfg.channels == CCP_MG_CHANNELS_BATCHED) {
        CCP_TRY(batched_levels(v, *h));
    } else {
        if (h->precision == CCP_MG_PRECISION_F32) CCP_TRY(narrow_levels(v, *h));
        CCP_TRY(nullspace_ready(v, *h));
    }
    *out = h;
    return CCP_OK;
}

// An operator that ccp_grid_refresh_weights_device installed has its verdict on the device: the synchronous calls read it
// (one wait) and refuse a poisoned operator before they touch x or b.  A setter's operator was validated on the host.
int refreshed_operator_ok(const GridMgView &v)
{
    if (!v.refreshed) return CCP_OK;
    unsigned word = 1;
    CCP_HIP(hipMemcpyAsync(&word, v.op_status, sizeof(word), hipMemcpyDeviceToHost, v.stream));
    CCP_HIP(hipStreamSynchronize(v.stream));
    return word ? CCP_ERR_STATE : CCP_OK;
}

// What ccp_grid_mg_apply (max_iteration 0) and the solve do alike before their first launch, in the handle's present
// configuration: the refusals, then vcycle_ready.
int call_ready(ccp_grid *g, int32_t max_iteration, int32_t smoothing_sweeps, GridMgView *v, int *nu, MgHierarchy **out)
{
    CCP_TRY(check_handle(g, v));
    CCP_TRY(sweeps_arg(smoothing_sweeps, nu, v->cfg.smoother));
    if (max_iteration < 0) return CCP_ERR_BAD_ARG;
    CCP_TRY(config_check(*v));
    CCP_TRY(refreshed_operator_ok(*v));
    return vcycle_ready(*v, out);
}

// Everything the solve does before its first launch: call_ready and the PCG work set of the channel mode.
int pcg_ready(ccp_grid *g, int32_t max_iteration, int32_t smoothing_sweeps, GridMgView *v, int *nu, MgHierarchy **out)
{
    CCP_TRY(call_ready(g, max_iteration, smoothing_sweeps, v, nu, out));
    const bool batched = v->cfg.channels == CCP_MG_CHANNELS_BATCHED;
    PcgArgs a{};                                                   // (the solve's shape: how many partial sums a channel needs)
    const long n = v->geom.ch_stride;                              // one channel incl. pads (pads stay 0 in every vector)
    a.shape(v->geom.W, v->geom.H, n, batched ? (unsigned)((v->channels + kMgbGroup - 1) / kMgbGroup) : 1);
    PcgWork &work = batched ? (*out)->bat : (*out)->seq;
    return work.alloc(batched ? v->channels : 1, n, std::max(a.apply_blocks, a.blocks), v->stream);
}

// The solve itself on what pcg_ready left: the mode's steps object, and its loop once (batched) or per channel.
// enqueue: the host-free form of the loop (pcg_enqueue), channel ch on the state h.estate[ch]; report is not used then.
// rel (enqueue only): the stop test relative to |b|, or null.
int pcg_solve(const GridMgView &v, MgHierarchy &h, double epsilon, int max_iteration, int nu, ccp_gs_report *report, bool enqueue,
              const PcgRelative *rel = nullptr)
{
    if (v.cfg.channels == CCP_MG_CHANNELS_BATCHED) return pcg_batched(v, h, epsilon, max_iteration, nu, report, enqueue, rel);
    const long n = v.geom.ch_stride;
    // one channel after the other: b, x, the channel's operator and, on the enqueue form, the channel's own state
    auto channels = [&](auto &S, auto &&each) -> int {
        S.h = &h, S.s = v.stream, S.epsilon = epsilon, S.nu = nu;
        S.shape(v.geom.W, v.geom.H, n);
        S.bind(h.seq, 0);
        for (int ch = 0; ch < v.channels; ++ch) {
            S.b = v.b + ch * n;
            S.x = v.x + ch * n;
            S.ch = ch;                                              // (one operator per channel: the channel's levels)
            each(ch);
            if (enqueue) {
                S.st = h.estate.p + ch;
                if (rel) rel->bind(S, ch);
                CCP_TRY(pcg_enqueue(S, max_iteration));
            } else {
                CgState host;
                CCP_TRY(pcg_loop(S, h, &host, 1, max_iteration, report ? report + ch : nullptr));
            }
        }
        return CCP_OK;
    };
    if (constant_mode(v)) {
        NullspaceSteps S{};
        S.lay = nullspace_layout(v), S.pixels = (double)v.geom.W * (double)v.geom.H;
        S.npart = h.nspart.p;
        S.hold = enqueue ? v.op_status : nullptr;
        CCP_TRY(channels(S, [&](int ch) {
            S.ns = h.nsstate.p + ch;
            v.ns->solved[ch] = false;
        }));
        if (enqueue) return CCP_OK;                                 // (the means stay on the device: k_mge_report reads them there)
        MgnState means[kMaxChannels] = {};                          // one read-back for all channels, after the last solve
        CCP_HIP(hipMemcpyAsync(means, h.nsstate.p, sizeof(MgnState) * (size_t)v.channels, hipMemcpyDeviceToHost, v.stream));
        CCP_HIP(hipStreamSynchronize(v.stream));
        for (int ch = 0; ch < v.channels; ++ch) {
            v.ns->solved[ch] = true;
            v.ns->b_mean[ch] = means[ch].b_mean;
            v.ns->x_mean[ch] = means[ch].x_mean;
        }
        return CCP_OK;
    }
    ChannelSteps S{};
    return channels(S, [](int) {});
}

// Is what the last ccp_grid_mg_prepare built what a solve of this view with `nu` sweeps runs on?
bool prepared_for(const GridMgView &v, const MgHierarchy *h, int nu)
{
    return h && h->prepared && h->estate.p && h->erel.p && cache_serves(v, *h) && h->prep_cfg == v.cfg && h->prep_nu == nu && h->prep_channels == v.channels;
}

// The two enqueue solves.  epsilon_rel null: ccp_grid_mg_conjugate_gradient_enqueue, the stop test against `epsilon` and
// the report of kMgeReportFields; otherwise ccp_grid_mg_conjugate_gradient_enqueue_relative, `epsilon` its epsilon_abs, the
// thresholds in h.erel and the report of kMgrReportFields.
int enqueue_solve(ccp_grid *g, double epsilon, const double *epsilon_rel, int32_t max_iteration, int32_t smoothing_sweeps,
                  const ccp_device_array *report)
{
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    int nu = 2;
    CCP_TRY(sweeps_arg(smoothing_sweeps, &nu, v.cfg.smoother));
    if (max_iteration < 0 || max_iteration > CCP_MG_ENQUEUE_MAX_ITERATION) return CCP_ERR_BAD_ARG;
    if (epsilon_rel)                                               // (the absolute call takes any epsilon, as the synchronous one)
        for (double e : {epsilon, *epsilon_rel})
            if (!(e >= 0.0) || std::isinf(e)) return CCP_ERR_BAD_ARG;
    const int fields = epsilon_rel ? kMgrReportFields : kMgeReportFields;
    if (report) CCP_TRY(check_view_on(v.device, report, 1u << CCP_DTYPE_F64, true, 1, v.channels, fields, 1));
    MgHierarchy *h = *v.cache;
    if (!prepared_for(v, h, nu)) return CCP_ERR_STATE;
    // The word and not what the host knows of it (v.refreshed): a recorded solve must see a refresh that follows the
    // recording, an eager one too.  0 while a setter's operator, validated on the host, is installed; null: not weighted.
    const unsigned *status = v.op_status;
    hipLaunchKernelGGL(k_mge_init, dim3(1), dim3(kBlock), 0, v.stream, h->estate.p, v.channels, status);
    double *const eps = h->erel.p, *const bnorm = eps + kMaxChannels;
    const PcgRelative rel{epsilon_rel ? *epsilon_rel : 0.0, eps, bnorm, bnorm + kMaxChannels, status};
    CCP_TRY(pcg_solve(v, *h, epsilon, max_iteration, nu, nullptr, true, epsilon_rel ? &rel : nullptr));
    if (report) {
        const MgeReport out{static_cast<double *>(const_cast<void *>(report->data)), (long)report->stride_y, (long)report->stride_x};
        const MgnState *ns = constant_mode(v) ? h->nsstate.p : nullptr;
        const CgState *st = h->estate.p;
        if (epsilon_rel)
            hipLaunchKernelGGL(k_mgr_report, dim3(1), dim3(kBlock), 0, v.stream, st, ns, v.channels, out, status, static_cast<const double *>(bnorm),
                               static_cast<const double *>(eps));
        else
            hipLaunchKernelGGL(k_mge_report, dim3(1), dim3(kBlock), 0, v.stream, st, ns, v.channels, out, status);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// ---- the options (ccp_grid_mg_set_* / _get_*) ---------------------------------------------------------------------------
// Every option takes the values 0 and 1 (CCP_MG_*_*, include/ccp_gs.h).  Per option: its place in MgConfig; when the
// setter returns CCP_ERR_UNSUPPORTED (null: never); what a change of value frees of a cached hierarchy (null: nothing).
// ccp_grid_mg_conjugate_gradient_enqueue rests on the last column: whatever is freed here is rebuilt by the next solve or
// prepare alone, so a change either deletes the hierarchy, or clears `prepared` with what it frees, or -- the null
// space, whose buffers serve both values -- frees nothing and leaves prepared_for to see that the options differ.
struct MgOption {
    int MgConfig::*field;
    bool (*unsupported)(const GridMgSlot &s, int value);
    void (*changed)(MgHierarchy **cache);
};
enum { kOptHierarchy, kOptPrecision, kOptChannels, kOptSmoother, kOptNullspace };

bool not_weighted(const GridMgSlot &s, int) { return !s.weighted; }

const MgOption kOptions[] = {
    // the cached levels belong to the other kind
    {&MgConfig::hierarchy, not_weighted, mg_release},
    // the cached vectors belong to the other precision; row blocks run the fp64 V-cycle only (local: nothing collective happens here)
    {&MgConfig::precision, [](const GridMgSlot &s, int value) { return value == CCP_MG_PRECISION_F32 && s.row_block; }, mg_release},
    // the other mode's vectors go; the levels stay
    {&MgConfig::channels, nullptr,
     [](MgHierarchy **cache) {
         batched_release(**cache);
         (*cache)->seq.release();
         (*cache)->prepared = false;
     }},
    // the line solves' work planes go; everything else is shared
    {&MgConfig::smoother, nullptr,
     [](MgHierarchy **cache) {
         (*cache)->lwork.release();
         (*cache)->lplane = 0;
         (*cache)->prepared = false;
     }},
    // the hierarchy and the PCG vectors serve both modes
    {&MgConfig::nullspace, not_weighted, nullptr},
};

// In this order: the handle, the value's range, the refusal (also of the value the handle holds), the same value (nothing happens)
int set_option(ccp_grid *g, int which, int32_t value)
{
    const MgOption &o = kOptions[which];
    GridMgSlot s{};
    CCP_TRY(grid_mg_slot(g, &s));
    if (value != 0 && value != 1) return CCP_ERR_BAD_ARG;
    if (o.unsupported && o.unsupported(s, value)) return CCP_ERR_UNSUPPORTED;
    if (s.cfg->*o.field == value) return CCP_OK;
    s.cfg->*o.field = value;
    if (o.changed && *s.cache) o.changed(s.cache);
    return CCP_OK;
}

int get_option(ccp_grid *g, int which, int32_t *value)
{
    GridMgSlot s{};
    CCP_TRY(grid_mg_slot(g, &s));
    if (!value) return CCP_ERR_BAD_ARG;
    *value = s.cfg->*kOptions[which].field;
    return CCP_OK;
}

}  // namespace

// ---- the hierarchy's half of ccp_grid_refresh_weights_device (ccp_grid_weighted.hip; ccp_grid_weighted_api.hpp) ---------
namespace {

// which of the mode-dependent verdicts a refresh of this view forms (config_check: batched channels are fp64, no null space)
struct RefreshPlan {
    bool f32, census;
};

RefreshPlan refresh_plan(const GridMgView &v, const MgHierarchy &h)
{
    const bool batched = v.cfg.channels == CCP_MG_CHANNELS_BATCHED;
    return RefreshPlan{!batched && h.precision == CCP_MG_PRECISION_F32, !batched && constant_mode(v)};
}

}  // namespace

// Is the handle one block with an operator, and is what the last ccp_grid_mg_prepare built still there and built for the
// handle's present options?  (Any smoothing_sweeps: no coefficient depends on them.)  CCP_ERR_STATE with nothing enqueued
// otherwise.
int ccp::mg_prepared(ccp_grid *g)
{
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    MgHierarchy *h = *v.cache;
    const bool ready = h && h->prepared && h->estate.p && cache_serves(v, *h) && h->prep_cfg == v.cfg && h->prep_channels == v.channels;
    return ready ? CCP_OK : CCP_ERR_STATE;
}

// mg_prepared, and if so the refresh's first launch: every word its kernels OR or count into, zeroed (n_counts of op_verdict)
int ccp::mg_refresh_begin(ccp_grid *g, int n_counts)
{
    CCP_TRY(mg_prepared(g));
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    MgHierarchy *h = *v.cache;
    const RefreshPlan plan = refresh_plan(v, *h);
    hipLaunchKernelGGL(k_mge_clear, dim3(1), dim3(kBlock), 0, v.stream, v.op_status, v.op_verdict, n_counts, plan.f32 ? h->fbad.p : nullptr,
                       plan.census ? h->nscount.p : nullptr);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// Level 0's planes hold new values (k_weighted_refresh is on the stream): everything derived from them again, by the
// launches that built it -- the coarse levels, the float copies, the census -- and the three verdicts folded into the
// status word.  Launches only; call after mg_refresh_begin said yes.
int ccp::mg_refresh(ccp_grid *g)
{
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    MgHierarchy &h = **v.cache;
    const bool f32 = refresh_plan(v, h).f32, census = refresh_plan(v, h).census;
    CCP_TRY(fill_levels(v, h));
    if (f32) CCP_TRY(narrow_launch(v, h));
    if (census) CCP_TRY(census_launch(v, h));
    hipLaunchKernelGGL(k_mge_status, dim3(1), dim3(kBlock), 0, v.stream, v.op_verdict, f32 ? static_cast<const unsigned *>(h.fbad.p) : nullptr,
                       census ? static_cast<const unsigned *>(h.nscount.p) : nullptr, v.op_channels, v.op_status);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

extern "C" {

int ccp_grid_mg_apply(ccp_grid *g, int32_t smoothing_sweeps)
try {
    GridMgView v{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(call_ready(g, 0, smoothing_sweeps, &v, &nu, &h));
    const long n = v.geom.ch_stride;
    if (constant_mode(v)) {                                        // x := z - mean(z), z = M (b - mean(b))
        NullspaceSteps S{};
        S.h = h, S.s = v.stream, S.nu = nu;
        S.shape(v.geom.W, v.geom.H, n);
        S.lay = nullspace_layout(v), S.pixels = (double)v.geom.W * (double)v.geom.H;
        S.ns = h->nsstate.p, S.npart = h->nspart.p;
        CCP_TRY(h->seq.alloc(1, n, 0, S.s));
        for (int ch = 0; ch < v.channels; ++ch) {
            S.b = v.b + ch * n, S.x = v.x + ch * n;
            S.means(S.b, nullptr, kMgnStart);                      // (m0 = 0)
            hipLaunchKernelGGL(k_mgn_center, dim3(S.blocks), dim3(kBlock), 0, S.s, S.b, h->seq.r.p, S.lay, static_cast<const MgnState *>(S.ns));
            CCP_TRY(vcycle(*h, S.s, h->seq.r.p, S.x, nu, nullptr, ch));
            CCP_TRY(S.finish());
        }
        CCP_HIP(hipGetLastError());
        CCP_HIP(hipStreamSynchronize(v.stream));
        return CCP_OK;
    }
    if (v.cfg.channels == CCP_MG_CHANNELS_BATCHED) {
        CCP_TRY(vcycle_batched(*h, v.stream, v.channels, n, v.b, v.x, nu, nullptr));
        CCP_HIP(hipStreamSynchronize(v.stream));
        return CCP_OK;
    }
    for (int ch = 0; ch < v.channels; ++ch) CCP_TRY(vcycle(*h, v.stream, v.b + ch * n, v.x + ch * n, nu, nullptr, ch));
    CCP_HIP(hipStreamSynchronize(v.stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_set_hierarchy(ccp_grid *g, int32_t kind) try { return set_option(g, kOptHierarchy, kind); } CCP_ABI_CATCH
int ccp_grid_mg_get_hierarchy(ccp_grid *g, int32_t *kind) try { return get_option(g, kOptHierarchy, kind); } CCP_ABI_CATCH
int ccp_grid_mg_set_precision(ccp_grid *g, int32_t precision) try { return set_option(g, kOptPrecision, precision); } CCP_ABI_CATCH
int ccp_grid_mg_get_precision(ccp_grid *g, int32_t *precision) try { return get_option(g, kOptPrecision, precision); } CCP_ABI_CATCH
int ccp_grid_mg_set_channels(ccp_grid *g, int32_t mode) try { return set_option(g, kOptChannels, mode); } CCP_ABI_CATCH
int ccp_grid_mg_get_channels(ccp_grid *g, int32_t *mode) try { return get_option(g, kOptChannels, mode); } CCP_ABI_CATCH
int ccp_grid_mg_set_smoother(ccp_grid *g, int32_t kind) try { return set_option(g, kOptSmoother, kind); } CCP_ABI_CATCH
int ccp_grid_mg_get_smoother(ccp_grid *g, int32_t *kind) try { return get_option(g, kOptSmoother, kind); } CCP_ABI_CATCH
int ccp_grid_mg_set_nullspace(ccp_grid *g, int32_t kind) try { return set_option(g, kOptNullspace, kind); } CCP_ABI_CATCH
int ccp_grid_mg_get_nullspace(ccp_grid *g, int32_t *kind) try { return get_option(g, kOptNullspace, kind); } CCP_ABI_CATCH

int ccp_grid_mg_nullspace_info(ccp_grid *g, int32_t channel, double *b_mean, double *x_mean, int64_t *pixels)
try {
    GridMgView v{};
    CCP_TRY(grid_mg_view(g, &v));
    if (channel < 0 || channel >= v.channels) return CCP_ERR_BAD_ARG;
    if (!v.weighted) return CCP_ERR_UNSUPPORTED;
    if (!v.ns->solved[channel]) return CCP_ERR_STATE;
    if (b_mean) *b_mean = v.ns->b_mean[channel];
    if (x_mean) *x_mean = v.ns->x_mean[channel];
    if (pixels) *pixels = (int64_t)v.geom.W * (int64_t)v.geom.H;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_debug_mgb_tile_lds(int32_t level_kind, int32_t smoothing_sweeps, int32_t *bytes, int32_t *threads)
try {
    if (level_kind < kMgSolve || level_kind > kMgCoarse || smoothing_sweeps < 1 || smoothing_sweeps > 4) return CCP_ERR_BAD_ARG;
    if (bytes) *bytes = tile_b_lds(level_kind, smoothing_sweeps);
    if (threads) *threads = mgb_tile_threads(level_kind);
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_level(ccp_grid *g, int32_t level, int32_t *n_levels, int32_t *width, int32_t *height, double *diag,
                      double *w_east, double *w_south)
try {
    return ccp_grid_mg_level_channel(g, 0, level, n_levels, width, height, diag, w_east, w_south);
} CCP_ABI_CATCH

int ccp_grid_mg_level_channel(ccp_grid *g, int32_t channel, int32_t level, int32_t *n_levels, int32_t *width, int32_t *height, double *diag,
                              double *w_east, double *w_south)
try {
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    if (channel < 0 || channel >= v.channels) return CCP_ERR_BAD_ARG;
    MgHierarchy *h = nullptr;
    CCP_TRY(hierarchy(v, &h));
    if (n_levels) *n_levels = h->levels;
    if (level < 0 || level >= h->levels) return CCP_ERR_BAD_ARG;
    const int oc = h->opC > 1 ? channel : 0;                       // the shared operator is every channel's
    const MgLevel &l = h->levels_of(oc)[level];
    if (width) *width = l.W;
    if (height) *height = l.H;
    if (!diag && !w_east && !w_south) return CCP_OK;
    const long n = (long)l.H * 2 * l.pitch;
    DevBuf<double> tmp;
    const double *src[3];
    if (level == 0) {
        CCP_TRY(tmp.alloc((size_t)(3 * n)));
        CCP_HIP(hipMemsetAsync(tmp.p, 0, sizeof(double) * 3 * n, v.stream));
        if (v.weighted) {                                          // the stored operator itself
            CCP_HIP(hipMemcpyAsync(tmp.p, l.d, sizeof(double) * n, hipMemcpyDeviceToDevice, v.stream));
            CCP_HIP(hipMemcpyAsync(tmp.p + n, l.we, sizeof(double) * n, hipMemcpyDeviceToDevice, v.stream));
            CCP_HIP(hipMemcpyAsync(tmp.p + 2 * n, l.ws, sizeof(double) * n, hipMemcpyDeviceToDevice, v.stream));
        } else if (v.masked)
            hipLaunchKernelGGL((k_mg_coef0<kMgMasked>), cells_grid(l.W, l.H), dim3(kBlock), 0, v.stream, l, tmp.p, tmp.p + n, tmp.p + 2 * n);
        else
            hipLaunchKernelGGL((k_mg_coef0<kMgSolve>), cells_grid(l.W, l.H), dim3(kBlock), 0, v.stream, l, tmp.p, tmp.p + n, tmp.p + 2 * n);
        CCP_HIP(hipGetLastError());
        for (int i = 0; i < 3; ++i) src[i] = tmp.p + i * n;
    } else {
        for (int i = 0; i < 3; ++i) src[i] = h->coef(oc, level, i);
    }
    double *dst[3] = {diag, w_east, w_south};
    std::vector<double> host((size_t)n);
    for (int i = 0; i < 3; ++i) {
        if (!dst[i]) continue;
        CCP_HIP(hipMemcpyAsync(host.data(), src[i], sizeof(double) * n, hipMemcpyDeviceToHost, v.stream));
        CCP_HIP(hipStreamSynchronize(v.stream));
        for (int y = 0; y < l.H; ++y)
            for (int x = 0; x < l.W; ++x) dst[i][(size_t)y * l.W + x] = host[(size_t)mg_at(l.pitch, x, y)];
    }
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_conjugate_gradient(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t smoothing_sweeps,
                                   ccp_gs_report *report)
try {
    GridMgView v{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(pcg_ready(g, max_iteration, smoothing_sweeps, &v, &nu, &h));
    return pcg_solve(v, *h, epsilon, max_iteration, nu, report, false);
} CCP_ABI_CATCH

int ccp_grid_mg_prepare(ccp_grid *g, int32_t smoothing_sweeps)
try {
    GridMgView v{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(pcg_ready(g, 0, smoothing_sweeps, &v, &nu, &h));
    h->prepared = false;
    if (!h->estate.p) CCP_TRY(h->estate.alloc((size_t)kMaxChannels));
    const bool batched = v.cfg.channels == CCP_MG_CHANNELS_BATCHED;
    const size_t rel_words = 2 * (size_t)kMaxChannels + (size_t)((batched ? v.channels : 1) * (batched ? h->bat : h->seq).ps);
    if (!h->erel.p || h->erel.n != rel_words) CCP_TRY(h->erel.alloc(rel_words));
    CCP_HIP(hipStreamSynchronize(v.stream));                       // what building enqueued has run: a failure shows here
    h->prep_cfg = v.cfg, h->prep_nu = nu, h->prep_channels = v.channels;
    h->prepared = true;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_conjugate_gradient_enqueue(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t smoothing_sweeps,
                                           const ccp_device_array *report)
try {
    return enqueue_solve(g, epsilon, nullptr, max_iteration, smoothing_sweeps, report);
} CCP_ABI_CATCH

int ccp_grid_mg_conjugate_gradient_enqueue_relative(ccp_grid *g, double epsilon_abs, double epsilon_rel, int32_t max_iteration,
                                                    int32_t smoothing_sweeps, const ccp_device_array *report)
try {
    return enqueue_solve(g, epsilon_abs, &epsilon_rel, max_iteration, smoothing_sweeps, report);
} CCP_ABI_CATCH

// ---- row blocks ----------------------------------------------------------------------------------------------------

int ccp_grid_mg_apply_rowblocked(ccp_grid *g, int32_t smoothing_sweeps)
try {
    GridMgView v{};
    Net net{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(prepare_rowblocked(g, smoothing_sweeps, true, &v, &net, &nu, &h));
    const MgLevel &l0 = h->lv[0];
    const long row = 2 * l0.pitch, n0 = (long)l0.H * row, n_own = (long)(l0.hi - l0.lo) * row;
    CCP_TRY(h->seq.alloc(1, n0, 0, net.s));               // (PCG work vectors in level 0's layout; zero beyond the owned rows)
    const long hoff = (long)v.geom.own_lo * row;
    for (int ch = 0; ch < v.channels; ++ch) {
        CCP_HIP(hipMemcpyAsync(h->seq.r.p + l0.lo * row, v.b + ch * v.geom.ch_stride + hoff, sizeof(double) * n_own, hipMemcpyDeviceToDevice, net.s));
        CCP_TRY(vcycle_rowblocked(*h, net, h->seq.r.p, h->seq.z.p, nu, nullptr));
        CCP_HIP(hipMemcpyAsync(v.x + ch * v.geom.ch_stride + hoff, h->seq.z.p + l0.lo * row, sizeof(double) * n_own, hipMemcpyDeviceToDevice, net.s));
    }
    CCP_HIP(hipStreamSynchronize(net.s));
    grid_mg_halo_stale(g);
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_rowblock_info(ccp_grid *g, int32_t *n_levels, int32_t *distributed_levels, int32_t *replicated_width,
                              int32_t *replicated_height)
try {
    GridMgView v{};
    Net net{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(prepare_rowblocked(g, 0, false, &v, &net, &nu, &h));
    CCP_HIP(hipStreamSynchronize(net.s));
    if (n_levels) *n_levels = h->levels;
    if (distributed_levels) *distributed_levels = h->dist;
    const bool any = h->dist < h->levels;
    if (replicated_width) *replicated_width = any ? h->lv[h->dist].W : 0;
    if (replicated_height) *replicated_height = any ? h->lv[h->dist].H : 0;
    return CCP_OK;
} CCP_ABI_CATCH

// The one-block PCG loop over the owned rows (RowSteps).  x is updated in place on the handle's owned rows (the owned
// range of a plane is laid out alike in the handle and in level 0).
int ccp_grid_mg_conjugate_gradient_rowblocked(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t smoothing_sweeps,
                                              ccp_gs_report *report)
try {
    if (max_iteration < 0) return CCP_ERR_BAD_ARG;
    GridMgView v{};
    Net net{};
    int nu = 2;
    MgHierarchy *h = nullptr;
    CCP_TRY(prepare_rowblocked(g, smoothing_sweeps, true, &v, &net, &nu, &h));
    const MgLevel &l0 = h->lv[0];
    const long row = 2 * l0.pitch, n0 = (long)l0.H * row, off = (long)l0.lo * row;
    const long n = (long)(l0.hi - l0.lo) * row;                       // the owned range (pads stay 0 in every vector)
    const long hoff = (long)v.geom.own_lo * row;
    RowSteps S{};
    S.h = h, S.s = net.s, S.epsilon = epsilon, S.nu = nu;
    S.net = &net;
    S.total = reinterpret_cast<double *>(net.comm->scratch.p);
    S.shape(l0.W, l0.hi - l0.lo, n);
    CCP_TRY(h->seq.alloc(1, n0, std::max(S.apply_blocks, S.blocks), S.s));
    S.bind(h->seq, off);
    for (int ch = 0; ch < v.channels; ++ch) {
        S.b = v.b + ch * v.geom.ch_stride + hoff;
        S.x = v.x + ch * v.geom.ch_stride + hoff;
        CgState host;
        CCP_TRY(pcg_loop(S, *h, &host, 1, max_iteration, report ? report + ch : nullptr));
    }
    grid_mg_halo_stale(g);                                                // the ghost rows of x are stale now
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"
