// ccp_grid_mg.hip — multigrid-preconditioned conjugate gradient on the grid handles (include/ccp_gs.h:
// ccp_grid_mg_*).  Kernels and the algorithm: ccp_grid_mg.hpp.
#include "ccp_grid_mg.hpp"

#include <algorithm>
#include <memory>
#include <vector>

using namespace ccp;

namespace ccp {

// The hierarchy of one handle: level 0 is the handle's own operator and vectors; levels 1.. own d, we, ws, b, z in
// one allocation (level layout, pads zero).  The PCG work vectors (one channel) are allocated at the first solve.
struct MgHierarchy {
    int levels = 0;
    int tail = 0;                    // first level of k_mg_tail (>= 1), or `levels` for a one-level hierarchy
    std::vector<MgLevel> lv;
    std::vector<long> base;          // per coarse level: offset of its d in `store` (then we, ws, b, z, t, each `size`)
    std::vector<long> size;
    DevBuf<double> store;
    DevBuf<double> t0;               // level 0's pre-smoothed z (one channel): k_mg_tile reads it while it writes z
    DevBuf<double> z, r, p, ap, partial;
    DevBuf<CgState> state;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int kind0 = kMgSolve;
    double *arr(int k, int which) { return store.p + base[k] + (long)which * size[k]; }   // 0 d, 1 we, 2 ws, 3 b, 4 z, 5 t
    ~MgHierarchy()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

void mg_release(MgHierarchy *h) { delete h; }

}  // namespace ccp

namespace {

dim3 cells_grid(int w, int h) { return dim3((unsigned)((w + kBlock - 1) / kBlock), (unsigned)h); }

template <int KIND>
void launch_coarsen(hipStream_t s, const MgLevel &f, const MgLevel &c, double *d, double *we, double *ws)
{
    hipLaunchKernelGGL((k_mg_coarsen<KIND>), cells_grid(c.W, c.H), dim3(kBlock), 0, s, f, c, d, we, ws);
}

int build(const GridMgView &v, MgHierarchy **out)
{
    MgHierarchy *h = new MgHierarchy();
    std::unique_ptr<MgHierarchy> own(h);
    h->kind0 = v.masked ? kMgMasked : kMgSolve;
    MgLevel l0{};
    l0.W = v.geom.W;
    l0.H = v.geom.H;
    l0.pitch = v.geom.pitch;
    l0.mask = v.mask;
    l0.g0 = v.geom;
    h->lv.push_back(l0);
    h->base.push_back(0);
    h->size.push_back(0);
    long total = 0;
    while (h->lv.back().W > 1 || h->lv.back().H > 1) {
        MgLevel c{};
        c.W = (h->lv.back().W + 1) / 2;
        c.H = (h->lv.back().H + 1) / 2;
        c.pitch = (((long)c.W + 1) / 2 + 15) / 16 * 16;
        h->lv.push_back(c);
        h->base.push_back(total);
        h->size.push_back((long)c.H * 2 * c.pitch);
        total += 6 * h->size.back();
    }
    h->levels = (int)h->lv.size();
    h->tail = h->levels;
    for (int k = 1; k < h->levels; ++k)
        if (h->lv[k].W <= kMgTailSide && h->lv[k].H <= kMgTailSide) {
            h->tail = k;
            break;
        }
    if (h->levels - h->tail > kMgTailLevels) return CCP_ERR_STATE;     // (cannot happen: sides <= 32 leave <= 6 levels)
    CCP_TRY(h->t0.alloc((size_t)v.geom.ch_stride));
    CCP_HIP(hipMemsetAsync(h->t0.p, 0, sizeof(double) * v.geom.ch_stride, v.stream));
    if (total > 0) {
        CCP_TRY(h->store.alloc((size_t)total));
        CCP_HIP(hipMemsetAsync(h->store.p, 0, sizeof(double) * total, v.stream));
    }
    for (int k = 1; k < h->levels; ++k) {
        h->lv[k].d = h->arr(k, 0);
        h->lv[k].we = h->arr(k, 1);
        h->lv[k].ws = h->arr(k, 2);
    }
    for (int k = 0; k + 1 < h->levels; ++k) {
        double *d = h->arr(k + 1, 0), *we = h->arr(k + 1, 1), *ws = h->arr(k + 1, 2);
        if (k > 0) launch_coarsen<kMgCoarse>(v.stream, h->lv[k], h->lv[k + 1], d, we, ws);
        else if (v.masked) launch_coarsen<kMgMasked>(v.stream, h->lv[0], h->lv[1], d, we, ws);
        else launch_coarsen<kMgSolve>(v.stream, h->lv[0], h->lv[1], d, we, ws);
        CCP_HIP(hipGetLastError());
    }
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return CCP_ERR_HIP;
    *out = own.release();
    return CCP_OK;
}

int hierarchy(const GridMgView &v, MgHierarchy **out)
{
    if (!*v.cache) CCP_TRY(build(v, v.cache));
    *out = *v.cache;
    return CCP_OK;
}

int sweeps_arg(int32_t smoothing_sweeps, int *nu)
{
    if (smoothing_sweeps < 0 || smoothing_sweeps > 4) return CCP_ERR_BAD_ARG;
    *nu = smoothing_sweeps == 0 ? 2 : smoothing_sweeps;
    return CCP_OK;
}

// one level above the tail: pre-smoothing and restriction (down), prolongation and post-smoothing (up)
dim3 tiles(const MgLevel &f) { return dim3((unsigned)((f.W + kMgTileW - 1) / kMgTileW), (unsigned)((f.H + kMgTileH - 1) / kMgTileH)); }

// t: the level's pre-smoothed z (restriction and the post-smoothing pass read it), z: its correction
template <int KIND>
void level_down(hipStream_t s, const MgLevel &f, const double *b, double *t, const MgLevel &c, double *bc, int nu, const CgState *st)
{
    hipLaunchKernelGGL((k_mg_tile<KIND, false>), tiles(f), dim3(kBlock), mg_tile_lds(nu), s, f, b, static_cast<const double *>(nullptr), t,
                       c, static_cast<const double *>(nullptr), nu, st);
    hipLaunchKernelGGL((k_mg_restrict<KIND>), cells_grid(c.W, c.H), dim3(kBlock), 0, s, f, b, t, c, bc, st);
}

template <int KIND>
void level_up(hipStream_t s, const MgLevel &f, const double *b, const double *t, double *z, const MgLevel &c, const double *ec, int nu,
              const CgState *st)
{
    hipLaunchKernelGGL((k_mg_tile<KIND, true>), tiles(f), dim3(kBlock), mg_tile_lds(nu), s, f, b, t, z, c, ec, nu, st);
}

// z0 := M^-1 b0 on level 0 (one channel); every launch is a no-op once st->active is 0 (st may be null)
int vcycle(MgHierarchy &h, hipStream_t s, const double *b0, double *z0, int nu, const CgState *st)
{
    auto B = [&](int k) -> const double * { return k ? h.arr(k, 3) : b0; };
    auto Z = [&](int k) -> double * { return k ? h.arr(k, 4) : z0; };
    auto T = [&](int k) -> double * { return k ? h.arr(k, 5) : h.t0.p; };
    if (h.levels == 1) {                                  // 1x1 image: z = b/d, what red updates from z = 0 give
        if (h.kind0 == kMgMasked)
            hipLaunchKernelGGL((k_mg_tile<kMgMasked, false>), dim3(1), dim3(kBlock), mg_tile_lds(nu), s, h.lv[0], b0, static_cast<const double *>(nullptr), z0, h.lv[0],
                               static_cast<const double *>(nullptr), nu, st);
        else
            hipLaunchKernelGGL((k_mg_tile<kMgSolve, false>), dim3(1), dim3(kBlock), mg_tile_lds(nu), s, h.lv[0], b0, static_cast<const double *>(nullptr), z0, h.lv[0],
                               static_cast<const double *>(nullptr), nu, st);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    for (int k = 0; k < h.tail; ++k) {
        double *bc = h.arr(k + 1, 3);
        if (k > 0) level_down<kMgCoarse>(s, h.lv[k], B(k), T(k), h.lv[k + 1], bc, nu, st);
        else if (h.kind0 == kMgMasked) level_down<kMgMasked>(s, h.lv[0], b0, T(0), h.lv[1], bc, nu, st);
        else level_down<kMgSolve>(s, h.lv[0], b0, T(0), h.lv[1], bc, nu, st);
    }
    MgTail t{};
    t.levels = h.levels - h.tail;
    int off = 0;
    for (int i = 0; i < t.levels; ++i) {
        const MgLevel &l = h.lv[h.tail + i];
        t.W[i] = l.W;
        t.H[i] = l.H;
        t.pitch[i] = l.pitch;
        t.off[i] = off;
        t.d[i] = l.d;
        t.we[i] = l.we;
        t.ws[i] = l.ws;
        off += l.W * l.H;
    }
    hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(kBlock), 0, s, t, B(h.tail), Z(h.tail), nu, st);
    for (int k = h.tail - 1; k >= 0; --k) {
        const double *ec = h.arr(k + 1, 4);
        if (k > 0) level_up<kMgCoarse>(s, h.lv[k], B(k), T(k), Z(k), h.lv[k + 1], ec, nu, st);
        else if (h.kind0 == kMgMasked) level_up<kMgMasked>(s, h.lv[0], b0, T(0), z0, h.lv[1], ec, nu, st);
        else level_up<kMgSolve>(s, h.lv[0], b0, T(0), z0, h.lv[1], ec, nu, st);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int check_handle(ccp_grid *g, GridMgView *v)
{
    CCP_TRY(grid_mg_view(g, v));
    if (!v->one_block) return CCP_ERR_STATE;
    return CCP_OK;
}

}  // namespace

extern "C" {

int ccp_grid_mg_apply(ccp_grid *g, int32_t smoothing_sweeps)
try {
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    int nu = 2;
    CCP_TRY(sweeps_arg(smoothing_sweeps, &nu));
    MgHierarchy *h = nullptr;
    CCP_TRY(hierarchy(v, &h));
    const long n = v.geom.ch_stride;
    for (int ch = 0; ch < v.channels; ++ch) CCP_TRY(vcycle(*h, v.stream, v.b + ch * n, v.x + ch * n, nu, nullptr));
    CCP_HIP(hipStreamSynchronize(v.stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_mg_level(ccp_grid *g, int32_t level, int32_t *n_levels, int32_t *width, int32_t *height, double *diag,
                      double *w_east, double *w_south)
try {
    GridMgView v{};
    CCP_TRY(check_handle(g, &v));
    MgHierarchy *h = nullptr;
    CCP_TRY(hierarchy(v, &h));
    if (n_levels) *n_levels = h->levels;
    if (level < 0 || level >= h->levels) return CCP_ERR_BAD_ARG;
    const MgLevel &l = h->lv[level];
    if (width) *width = l.W;
    if (height) *height = l.H;
    if (!diag && !w_east && !w_south) return CCP_OK;
    const long n = (long)l.H * 2 * l.pitch;
    DevBuf<double> tmp;
    const double *src[3];
    if (level == 0) {
        CCP_TRY(tmp.alloc((size_t)(3 * n)));
        CCP_HIP(hipMemsetAsync(tmp.p, 0, sizeof(double) * 3 * n, v.stream));
        if (v.masked)
            hipLaunchKernelGGL((k_mg_coef0<kMgMasked>), cells_grid(l.W, l.H), dim3(kBlock), 0, v.stream, l, tmp.p, tmp.p + n, tmp.p + 2 * n);
        else
            hipLaunchKernelGGL((k_mg_coef0<kMgSolve>), cells_grid(l.W, l.H), dim3(kBlock), 0, v.stream, l, tmp.p, tmp.p + n, tmp.p + 2 * n);
        CCP_HIP(hipGetLastError());
        for (int i = 0; i < 3; ++i) src[i] = tmp.p + i * n;
    } else {
        for (int i = 0; i < 3; ++i) src[i] = h->arr(level, i);
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
    CCP_TRY(check_handle(g, &v));
    int nu = 2;
    CCP_TRY(sweeps_arg(smoothing_sweeps, &nu));
    if (max_iteration < 0) return CCP_ERR_BAD_ARG;
    MgHierarchy *h = nullptr;
    CCP_TRY(hierarchy(v, &h));
    const Geom &geo = v.geom;
    const long n = geo.ch_stride;                                  // one channel incl. pads (pads stay 0 in every vector)
    // k_mg_apply: rows folded so that the grid has ~2,048 blocks (and as many partial sums for k_cg_alpha)
    const unsigned agx = cells_grid((geo.W + 1) / 2, 1).x;
    const dim3 agrid(agx, (unsigned)std::max(1, std::min(geo.H, (int)(1024 / agx))), 2);
    const int apply_blocks = (int)(agrid.x * agrid.y * agrid.z);
    const int blocks = (int)std::max<long>(1, std::min<long>(2048, (n + kBlock - 1) / kBlock));
    hipStream_t s = v.stream;
    if (!h->z.p) {
        CCP_TRY(h->z.alloc((size_t)n));
        CCP_TRY(h->r.alloc((size_t)n));
        CCP_TRY(h->p.alloc((size_t)n));
        CCP_TRY(h->ap.alloc((size_t)n));
        CCP_TRY(h->partial.alloc((size_t)std::max(apply_blocks, blocks)));
        CCP_TRY(h->state.alloc(1));
        for (DevBuf<double> *b : {&h->z, &h->r, &h->p, &h->ap}) CCP_HIP(hipMemsetAsync(b->p, 0, sizeof(double) * n, s));
    }
    CgState *st = h->state.p;
    double *part = h->partial.p;
    const MgLevel &l0 = h->lv[0];
    auto apply = [&](const double *in, double *out, bool dot) {           // the product of an iteration stops with the loop
        if (v.masked) {
            if (dot) hipLaunchKernelGGL((k_mg_apply<kMgMasked, true>), agrid, dim3(kBlock), 0, s, l0, in, out, part, st);
            else hipLaunchKernelGGL((k_mg_apply<kMgMasked, false>), agrid, dim3(kBlock), 0, s, l0, in, out, part, static_cast<const CgState *>(nullptr));
        } else {
            if (dot) hipLaunchKernelGGL((k_mg_apply<kMgSolve, true>), agrid, dim3(kBlock), 0, s, l0, in, out, part, st);
            else hipLaunchKernelGGL((k_mg_apply<kMgSolve, false>), agrid, dim3(kBlock), 0, s, l0, in, out, part, static_cast<const CgState *>(nullptr));
        }
    };
    for (int ch = 0; ch < v.channels; ++ch) {
        const double *b = v.b + ch * n;
        double *x = v.x + ch * n;
        CgState host{};
        host.active = 1;
        CCP_HIP(hipMemcpyAsync(st, &host, sizeof(host), hipMemcpyHostToDevice, s));
        CCP_HIP(hipEventRecord(h->ev0, s));
        apply(x, h->r.p, false);                                                              // r = A x
        hipLaunchKernelGGL(k_cg_init, dim3(blocks), dim3(kBlock), 0, s, b, h->r.p, h->p.p, n, part);   // r = b - r; r'r
        hipLaunchKernelGGL(k_mg_check, dim3(1), dim3(kBlock), 0, s, part, blocks, epsilon, st);
        CCP_TRY(vcycle(*h, s, h->r.p, h->z.p, nu, st));                                   // z = M r
        hipLaunchKernelGGL(k_cg_dot, dim3(blocks), dim3(kBlock), 0, s, h->r.p, h->z.p, n, part, st);
        hipLaunchKernelGGL(k_cg_set_rlen, dim3(1), dim3(kBlock), 0, s, part, blocks, st);   // rlen = r'z
        CCP_HIP(hipMemcpyAsync(h->p.p, h->z.p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));   // p = z
        CCP_HIP(hipGetLastError());
        CCP_HIP(hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s));
        CCP_HIP(hipStreamSynchronize(s));
        int issued = 0;
        bool active = host.active != 0 && max_iteration > 0;
        while (active && issued < max_iteration) {
            const int batch = std::min(16, max_iteration - issued);
            for (int k = 0; k < batch; ++k) {
                apply(h->p.p, h->ap.p, true);                                                // Ap, p'Ap partials
                hipLaunchKernelGGL(k_cg_alpha, dim3(1), dim3(kBlock), 0, s, part, apply_blocks, st);   // alpha = r'z / p'Ap
                hipLaunchKernelGGL(k_cg_update, dim3(blocks), dim3(kBlock), 0, s, x, h->p.p, h->r.p, h->ap.p, n, part, st);
                hipLaunchKernelGGL(k_mg_check, dim3(1), dim3(kBlock), 0, s, part, blocks, epsilon, st);
                CCP_TRY(vcycle(*h, s, h->r.p, h->z.p, nu, st));
                hipLaunchKernelGGL(k_cg_dot, dim3(blocks), dim3(kBlock), 0, s, h->r.p, h->z.p, n, part, st);
                hipLaunchKernelGGL(k_mg_beta, dim3(1), dim3(kBlock), 0, s, part, blocks, st);
                hipLaunchKernelGGL(k_cg_direction, dim3(blocks), dim3(kBlock), 0, s, h->p.p, h->z.p, n, st);   // p = z + beta p
            }
            CCP_HIP(hipGetLastError());
            issued += batch;
            CCP_HIP(hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s));
            CCP_HIP(hipStreamSynchronize(s));
            active = host.active != 0;
        }
        CCP_HIP(hipEventRecord(h->ev1, s));
        CCP_HIP(hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s));
        CCP_HIP(hipStreamSynchronize(s));
        if (report) {
            float ms = 0.f;
            CCP_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
            report[ch].iterations = host.iterations;
            report[ch].converged = host.converged;
            report[ch].last_l1_step = host.r1norm;
            report[ch].seconds = ms * 1e-3;
        }
    }
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"
