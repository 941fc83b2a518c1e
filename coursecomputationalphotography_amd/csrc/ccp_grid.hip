// ccp_grid.hip — C ABI of the structured (matrix-free) Poisson grid path: the handle's life cycle, the red-black
// passes and the Gauss-Seidel, conjugate-gradient and row-block solves.  See include/ccp_gs.h; the handle itself is in
// ccp_grid_handle.hpp, the rest of its calls in ccp_grid_lex.hip, ccp_grid_io.hip and ccp_grid_weighted.hip.
#include "ccp_grid_handle.hpp"
#include "ccp_grid_kernels.hpp"
#include "ccp_grid_fused.hpp"
#include "ccp_grid_fused_wide.hpp"
#include "ccp_cg.hpp"
#include "ccp_grid_cg.hpp"
#include "ccp_grid_mg_view.hpp"
#include "ccp_comm.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace ccp;

// ---- what the handle's other translation units call too (ccp_grid_handle.hpp) ----
namespace ccp {

// Did a polling kernel give up on the edge flag (see ccp_grid::edge_timeout)?
int edge_timeout_status(const ccp_grid *g)
{
    if (g->edge_timeout && __atomic_load_n(g->edge_timeout, __ATOMIC_ACQUIRE) != 0) {
        if (getenv("CCP_GS_DEBUG")) fprintf(stderr, "[ccp_gs] an edge hand-off timed out: ghost rows may hold rows that were not final\n");
        return CCP_ERR_STATE;
    }
    return CCP_OK;
}

int bind(ccp_grid *g)
{
    if (!g) return CCP_ERR_BAD_ARG;
    if (hipSetDevice(g->device) != hipSuccess) return CCP_ERR_NO_DEVICE;
    return edge_timeout_status(g);
}

// The calls a weighted handle refuses (sweeps, Gauss-Seidel, plain CG, tuning, SolveChannel assembly, region blends,
// masks, row blocks): include/ccp_gs.h, CCP_GRID_WEIGHTED
int not_weighted(const ccp_grid *g)
{
    if (!g) return CCP_ERR_BAD_ARG;
    return g->weighted ? CCP_ERR_UNSUPPORTED : CCP_OK;
}

}  // namespace ccp

namespace {

long sweep_blocks_x(const ccp_grid *g) { return (g->geom.pitch + (long)kBlock * g->cpt - 1) / ((long)kBlock * g->cpt); }

void choose_tiling(ccp_grid *g)
{
    // Aim for >= 4096 workgroups (>> 256 CUs x 8 resident blocks) while keeping the
    // two-row halo re-read per row tile small.
    const long bx = sweep_blocks_x(g);
    long r = (long)g->geom.local_rows * bx * g->desc.channels / 4096;
    r = std::max<long>(4, std::min<long>(64, r));
    g->rows_per_block = (int)r;
}

template <bool L1>
int launch_half_sweep(ccp_grid *g, int c, int l_lo, int l_hi, const int *active)
{
    if (l_hi <= l_lo) return CCP_OK;
    const Geom &geo = g->geom;
    const int rpb = g->rows_per_block;
    dim3 grid((unsigned)sweep_blocks_x(g), (unsigned)((l_hi - l_lo + rpb - 1) / rpb), (unsigned)g->desc.channels);
    dim3 block(kBlock);
    double *part = g->partial.p + (long)c * g->partial_region;
#define CCP_LAUNCH_SWEEP(CPT_, SHFL_)                                                                          \
    hipLaunchKernelGGL((k_half_sweep<CPT_, L1, SHFL_>), grid, block, 0, g->stream, g->x.p, g->x.p, g->b.p, geo, \
                       c, l_lo, l_hi, rpb, part, active, static_cast<const unsigned char *>(nullptr))
    if (g->masked) {
        hipLaunchKernelGGL((k_half_sweep<2, L1, true, true>), grid, block, 0, g->stream, g->x.p, g->x.p, g->b.p, geo, c, l_lo, l_hi,
                           rpb, part, active, g->maskp.p);
    } else {
        CCP_LAUNCH_SWEEP(2, true);
    }
#undef CCP_LAUNCH_SWEEP
    CCP_HIP(hipGetLastError());
    g->last_launches++;
    g->region_launches++;
    return CCP_OK;
}

// Rows a half-sweep may update: everything on a side that is the image border, and on a side
// with ghosts one row fewer per half-sweep since the last halo refresh.
void sweep_range(const ccp_grid *g, int &l_lo, int &l_hi)
{
    const int s = g->half_sweeps_since_refresh;
    l_lo = g->shrink_top ? std::min(s + 1, g->ghost_top) : 0;
    l_hi = g->geom.local_rows - (g->shrink_bottom ? std::min(s + 1, g->ghost_bottom) : 0);
}

long l1_blocks_per_colour_channel(const ccp_grid *g, int l_lo, int l_hi)
{
    const int rpb = g->rows_per_block;
    return sweep_blocks_x(g) * (long)((l_hi - l_lo + rpb - 1) / rpb);
}

// blocks_out[c]: L1 block results per channel the colour-c half-sweep wrote.
int one_iteration(ccp_grid *g, bool l1, const int *active, long *blocks_out)
{
    for (int c = 0; c < 2; ++c) {
        int lo, hi;
        sweep_range(g, lo, hi);
        if ((g->shrink_top || g->shrink_bottom) && g->half_sweeps_since_refresh >= g->desc.ghost)
            return CCP_ERR_STATE;   // ghosts exhausted: refresh the halo first
        if (l1) {
            CCP_TRY(launch_half_sweep<true>(g, c, lo, hi, active));
            if (blocks_out) blocks_out[c] = l1_blocks_per_colour_channel(g, lo, hi);
        } else {
            CCP_TRY(launch_half_sweep<false>(g, c, lo, hi, active));
        }
        if (g->shrink_top || g->shrink_bottom) g->half_sweeps_since_refresh++;
    }
    return CCP_OK;
}

// The handle as the pass planner sees it (ccp_fused_plan.hpp), with the chunk height in force at depth T.
FusedPlanInput plan_input(const ccp_grid *g, int T)
{
    FusedPlanInput in;
    in.g = g->geom;
    in.stale_top = g->shrink_top;
    in.stale_bottom = g->shrink_bottom;
    in.ghost = g->desc.ghost;
    in.ghost_top = g->ghost_top;
    in.ghost_bottom = g->ghost_bottom;
    in.send_up = g->send_up;
    in.send_down = g->send_down;
    in.channels = g->desc.channels;
    in.cus = g->cus;
    in.rows_per_chunk = (g->tuned && g->tune_rows[T] > 0) ? g->tune_rows[T] : g->rows_per_chunk;
    in.short_edges = g->short_edges;
    in.all_border = g->all_border;
    in.side_rows_override = g->side_rows_override;
    in.wide = g->wide;
    in.wide_segments = g->wide_segments;
    return in;
}

// One planned pass: all a launcher needs beside the handle.
// l1: 0 none, 1 step of the last sweep, 2 step of every sweep of the pass; l1_blocks[0/1]: block results per
// (sweep, channel) of the ordinary / the border launch.
// store_red = false: the ordinary tiles of an unchecked pass store only the black halves (fused_wave says when that is
// safe; run_unchecked decides); border tiles, checked and edge passes always store both.
struct FusedPass {
    FusedPlan plan;
    const double *xin = nullptr;
    double *xout = nullptr;
    const int *active = nullptr;
    int l1 = 0;
    long *l1_blocks = nullptr;
    bool store_red = true;
};

// Plans the pass `kind` (depth, rows, l1, multi) on this handle.  edge_rows > 0: the EDGE kernels (edge chunks first,
// in-launch signal) where the pass can signal by itself: unchecked, every channel, a counter to count in.
FusedPass plan_pass(const ccp_grid *g, FusedPassKind kind, const int *active = nullptr, int edge_rows = 0)
{
    kind.masked = g->masked;
    kind.edge_rows = (edge_rows > 0 && kind.l1 == 0 && active == nullptr && g->edge_counter && g->edge_signal) ? edge_rows : 0;
    FusedPass pass;
    pass.plan = fused_plan(plan_input(g, kind.T), kind);
    pass.active = active;
    pass.l1 = kind.l1;
    return pass;
}

// The kernels' argument: the plan's tiling and the handle's buffers (no hand-off, no trace).
FusedParams fused_params(const ccp_grid *g, const FusedPass &pass)
{
    const FusedPlan &L = pass.plan;
    FusedParams P{};
    P.xin = pass.xin;
    P.xout = pass.xout;
    P.b = g->b.p;
    P.g = g->geom;
    P.st_lo = L.st_lo;
    P.st_hi = L.st_hi;
    P.rows_per_chunk = L.rows_per_chunk;
    P.first_rows = L.first_rows;
    P.last_rows = L.last_rows;
    P.n_strips = L.n_strips;
    P.partial = g->partial.p;
    P.active = pass.active;
    P.n_chunks = L.n_chunks;
    P.nb_top = L.nb_top;
    P.nb_bot = L.nb_bot;
    P.ns_left = L.ns_left;
    P.ns_right = L.ns_right;
    P.side_rows = L.side_rows;
    P.side_subs = L.side_subs;
    P.side_rows_edge = L.side_rows_edge;
    P.partial_border = g->partial.p + g->partial_region;
    P.mask = g->maskp.p;
    P.first_edge = L.first_edge;
    P.last_edge = L.last_edge;
    P.xcd_swizzle = g->xcd_swizzle ? 1 : 0;
    P.wide_y0 = L.wide_y0;
    P.wide_y1 = L.wide_y1;
    P.wide_h = L.wide_h;
    P.wide_nseg = L.wide_nseg;
    P.wide_stride = L.wide_stride;
    P.wide_tiles = L.wide_tiles;
    return P;
}

void report_l1_blocks(const FusedPass &pass)
{
    if (!pass.l1_blocks) return;
    const FusedPlan &L = pass.plan;
    pass.l1_blocks[0] = L.any_plain ? (long)L.grid_x * L.grid_y : 0;
    pass.l1_blocks[1] = L.n_border ? (long)L.bgrid_x : 0;
}


// Which tiles of a Dirichlet-mask grid hold unknowns: one census per tiling (depth, chunk rows, row range).
int masked_tile_census(ccp_grid *g, const FusedParams &P, int T)
{
    if (g->live_T != T || g->live_R != P.rows_per_chunk || g->live_lo != P.st_lo || g->live_hi != P.st_hi) {
        const size_t tiles = (size_t)P.n_chunks * P.n_strips;
        if (g->tile_live.n < tiles) CCP_TRY(g->tile_live.alloc(tiles));
        if (g->tile_rows.n < 2 * tiles) CCP_TRY(g->tile_rows.alloc(2 * tiles));
        hipLaunchKernelGGL(k_masked_tile_census, dim3((unsigned)P.n_strips, (unsigned)P.n_chunks), dim3(kWave), 0, g->stream, P, T,
                           g->tile_live.p, g->tile_rows.p);
        CCP_HIP(hipGetLastError());
        g->live_T = T;
        g->live_R = P.rows_per_chunk;
        g->live_lo = P.st_lo;
        g->live_hi = P.st_hi;
    }
    return CCP_OK;
}

// One pass of depth T over a Dirichlet-mask grid: every tile is an ordinary tile (zero lies outside the block
// as it does outside the region), tiles without any unknown in reach leave at once.
template <int T>
int launch_fused_masked(ccp_grid *g, const FusedParams &P, const FusedPass &pass)
{
    if (T > kMaskedMaxT) return CCP_ERR_BAD_ARG;
    constexpr int TM = T <= kMaskedMaxT ? T : 1;
    const int l1 = pass.l1;
    const dim3 grid(pass.plan.grid_x, pass.plan.grid_y, (unsigned)g->desc.channels);
    report_l1_blocks(pass);
    CCP_TRY(masked_tile_census(g, P, T));
    static const bool clip_rows = !(getenv("CCP_GS_MASK_ROWS") && atoi(getenv("CCP_GS_MASK_ROWS")) == 0);   // A/B: march every row of a live tile
    const int *rows_p = clip_rows ? g->tile_rows.p : nullptr;
    if (l1 == 2 && T > kMaskedMaxCheckedT) return CCP_ERR_BAD_ARG;
    constexpr int TMC = T <= kMaskedMaxCheckedT ? T : 1;
    if (l1 == 2) hipLaunchKernelGGL((k_fused_sweep_masked<TMC, 2, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P, g->tile_live.p, rows_p);
    else if (l1 == 1) hipLaunchKernelGGL((k_fused_sweep_masked<TM, 1, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P, g->tile_live.p, rows_p);
    else if (!pass.store_red) hipLaunchKernelGGL((k_fused_sweep_masked<TM, 0, kFusedUnroll, false>), grid, dim3(kBlock), 0, g->stream, P, g->tile_live.p, rows_p);
    else hipLaunchKernelGGL((k_fused_sweep_masked<TM, 0, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P, g->tile_live.p, rows_p);
    CCP_HIP(hipGetLastError());
    g->last_launches++;
    g->region_launches++;
    g->region_iterations += T;
    return CCP_OK;
}

// One pass of depth T = pass.plan.T: the kernels' argument from the plan, the instantiation, the launches on two streams.
template <int T>
int launch_fused_t(ccp_grid *g, const FusedPass &pass)
{
    const FusedPlan &L = pass.plan;
    const int l1 = pass.l1;
    FusedParams P = fused_params(g, pass);
    if (g->masked) return launch_fused_masked<T>(g, P, pass);
    const int waves = kBlock / kWave;
    const long n_border = L.n_border;
    const bool any_plain = L.any_plain, edge = L.edge, wide = L.wide, store_red = pass.store_red;
    const dim3 grid(L.grid_x, L.grid_y, (unsigned)g->desc.channels);
    const dim3 bgrid(L.bgrid_x, 1, (unsigned)g->desc.channels);
    const dim3 wgrid(L.wgrid_x, 1, 1);
    report_l1_blocks(pass);
    if (l1 == 2 && T > kFusedMaxCheckedT) return CCP_ERR_BAD_ARG;
    P.edge_counter = g->edge_counter;
    P.edge_flag = g->edge_flag;
    P.edge_epoch = g->edge_epoch;
    P.edge_target = L.edge_target;
    if (edge) {
        // every edge pass counts from zero in a ring slot of its own (a miscount can cost one overlap, never
        // the next); the whole ring is cleared once per kEdgeRing epochs, off the critical path of a pass
        if (g->edge_epoch % kEdgeRing == 0) CCP_HIP(hipMemsetAsync(g->edge_counter, 0, sizeof(unsigned long long) * kEdgeRing, g->stream));
        P.edge_counter = g->edge_counter + (g->edge_epoch % kEdgeRing);
    }
    const dim3 pgrid = wide ? wgrid : grid;                   // the ordinary launch
    // diagnostics: per-wave time stamps of this pass (ordinary launch first, border launch behind it)
    const size_t trace_plain = (size_t)pgrid.x * pgrid.y * pgrid.z * waves * 4, trace_border = (size_t)bgrid.x * bgrid.z * waves * 4;
    unsigned long long *trace_p = nullptr, *trace_b = nullptr;
    if (g->trace_file) {
        if (g->trace.n < trace_plain + trace_border) CCP_TRY(g->trace.alloc(trace_plain + trace_border));
        CCP_HIP(hipMemsetAsync(g->trace.p, 0, (trace_plain + trace_border) * sizeof(unsigned long long), g->stream));
        trace_p = g->trace.p;
        trace_b = g->trace.p + trace_plain;
    }
    P.trace = trace_b;
    constexpr int TC = T <= kFusedMaxCheckedT ? T : 1;       // per-sweep sums exist up to kFusedMaxCheckedT
    hipStream_t bstream = g->stream2;
    // The border launch sees everything queued on the main stream so far, runs beside the ordinary
    // tiles, and whatever comes next on the main stream waits for it.
    if (n_border) {
        CCP_HIP(hipEventRecord(g->ev_main, g->stream));
        CCP_HIP(hipStreamWaitEvent(bstream, g->ev_main, 0));
    }
    // an EDGE pass issues its border tiles first: the few side-strip waves of the edge chunks must not queue
    // behind a chip full of ordinary tiles, or the hand-off would come at the end of the pass
    if (n_border && edge) {
        hipLaunchKernelGGL((k_fused_border<T, 0, kFusedUnroll, true>), bgrid, dim3(kBlock), 0, bstream, P, g->force_border ? 1 : 0);
    }
    if (any_plain) {
        P.trace = trace_p;
        if (l1 == 2) hipLaunchKernelGGL((k_fused_sweep<TC, 2, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P);
        else if (l1 == 1) hipLaunchKernelGGL((k_fused_sweep<T, 1, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P);
        else if (edge) hipLaunchKernelGGL((k_fused_sweep<T, 0, kFusedUnroll, true>), grid, dim3(kBlock), 0, g->stream, P);
        else if (wide && !store_red) hipLaunchKernelGGL((k_fused_sweep_wide<kWideT, false>), wgrid, dim3(kBlock), 0, g->stream, P, L.wx0, L.wx1, L.n_wide);
        else if (wide) hipLaunchKernelGGL((k_fused_sweep_wide<kWideT, true>), wgrid, dim3(kBlock), 0, g->stream, P, L.wx0, L.wx1, L.n_wide);
        else if (!store_red) hipLaunchKernelGGL((k_fused_sweep<T, 0, kFusedUnroll, false, false>), grid, dim3(kBlock), 0, g->stream, P);
        else hipLaunchKernelGGL((k_fused_sweep<T, 0, kFusedUnroll>), grid, dim3(kBlock), 0, g->stream, P);
    }
    if (n_border) {
        const int fb = g->force_border ? 1 : 0;
        P.trace = trace_b;
        if (l1 == 2) hipLaunchKernelGGL((k_fused_border<TC, 2, kFusedUnroll>), bgrid, dim3(kBlock), 0, bstream, P, fb);
        else if (l1 == 1) hipLaunchKernelGGL((k_fused_border<T, 1, kFusedUnroll>), bgrid, dim3(kBlock), 0, bstream, P, fb);
        else if (!edge) hipLaunchKernelGGL((k_fused_border<T, 0, kFusedUnroll>), bgrid, dim3(kBlock), 0, bstream, P, fb);
        CCP_HIP(hipEventRecord(g->ev_side, bstream));
        CCP_HIP(hipStreamWaitEvent(g->stream, g->ev_side, 0));
    }
    CCP_HIP(hipGetLastError());
    if (g->trace_file) {
        CCP_HIP(hipStreamSynchronize(g->stream));
        std::vector<unsigned long long> host(trace_plain + trace_border);
        CCP_HIP(hipMemcpy(host.data(), g->trace.p, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(g->trace_file, "ab")) {
            const unsigned long long head[8] = {0x43435054524143ull, (unsigned long long)T, pgrid.x, pgrid.y, pgrid.z, bgrid.x, (unsigned long long)host.size(),
                                                (unsigned long long)P.rows_per_chunk};
            fwrite(head, sizeof(head), 1, f);
            fwrite(host.data(), sizeof(unsigned long long), host.size(), f);
            fclose(f);
        }
    }
    g->last_launches++;
    g->region_launches++;
    g->region_iterations += T;
    return CCP_OK;
}

// `n_passes` passes of one depth as ONE launch (k_fused_multi): xin -> xout -> xin ...  `first` is pass 0, planned with
// FusedPassKind::multi: its tiling serves the whole group; st_lo / st_hi: the rows each pass stores.
// red_skip: the first red_skip passes store only the black halves in their ordinary tiles (FusedPass::store_red).
struct FusedMultiPass {
    FusedPass first;
    int n_passes = 0;
    int st_lo[kMultiMaxPasses], st_hi[kMultiMaxPasses];
    int red_skip = 0;
};

// Returns CCP_ERR_UNSUPPORTED when the shape does not qualify (the caller then issues the passes one by one).
template <int T>
int launch_fused_multi_t(ccp_grid *g, const FusedMultiPass &group)
{
    const int n_passes = group.n_passes;
    if (n_passes < 2 || n_passes > kMultiMaxPasses || g->trace_file) return CCP_ERR_UNSUPPORTED;
    if (g->masked && T > kMaskedMaxT) return CCP_ERR_UNSUPPORTED;
    const FusedPlan &L = group.first.plan;
    FusedMultiParams M{};
    FusedParams &P = M.P;
    P = fused_params(g, group.first);
    P.xcd_swizzle = 0;
    const int HS = 2 * T;
    if (g->masked) CCP_TRY(masked_tile_census(g, P, T));
    // a tile waits for the tiles two chunks up and down: of any two adjacent chunks at least one must be as tall
    // as the halo (2T rows) — true when the regular and the special chunk heights are, whatever the remainder chunk
    if (P.rows_per_chunk < HS || (P.first_rows > 0 && P.first_rows < HS) || (P.last_rows > 0 && P.last_rows < HS)) return CCP_ERR_UNSUPPORTED;
    for (int c = 0; c + 1 < P.n_chunks; ++c) {
        int ra, rb, rc, rd;
        fused_chunk_rows(P, c, ra, rb);
        fused_chunk_rows(P, c + 1, rc, rd);
        if (rb - ra < HS && rd - rc < HS) return CCP_ERR_UNSUPPORTED;
    }
    for (int q = 0; q < n_passes; ++q) {
        if (group.st_hi[q] <= group.st_lo[q] || group.st_lo[q] < group.st_lo[0] || group.st_hi[q] > group.st_hi[0]) return CCP_ERR_UNSUPPORTED;
        M.st_lo[q] = group.st_lo[q];
        M.st_hi[q] = group.st_hi[q];
    }
    M.n_passes = n_passes;
    M.red_skip = group.red_skip;
    M.gx = (int)L.grid_x;
    M.gy = (int)L.grid_y;
    M.bgx = (int)L.bgrid_x;
    M.channels = g->desc.channels;
    const size_t cells = (size_t)n_passes * M.channels * P.n_chunks * P.n_strips;
    if (g->multi_words.n < cells + 2) CCP_TRY(g->multi_words.alloc(cells + 2));
    CCP_HIP(hipMemsetAsync(g->multi_words.p, 0, (cells + 2) * sizeof(unsigned), g->stream));
    M.ticket = g->multi_words.p;
    M.cells = g->multi_words.p + 2;
    M.error = g->edge_timeout;
    M.tile_live = g->tile_live.p;
    const long total = (long)n_passes * (M.bgx + (long)M.gx * M.gy) * M.channels;
    if (total > 0x7fffffffL) return CCP_ERR_UNSUPPORTED;
    constexpr int TM = T <= kMaskedMaxT ? T : 1;
    if (g->masked) hipLaunchKernelGGL((k_fused_multi<TM, kFusedUnroll, true>), dim3((unsigned)total), dim3(kBlock), 0, g->stream, M);
    else hipLaunchKernelGGL((k_fused_multi<T, kFusedUnroll>), dim3((unsigned)total), dim3(kBlock), 0, g->stream, M);
    CCP_HIP(hipGetLastError());
    g->last_launches += n_passes;
    g->region_launches += n_passes;
    g->region_iterations += (long)T * n_passes;
    return CCP_OK;
}

// run-time depth (the plan's) -> the instantiation of that depth
template <int TMAX>
struct FusedDepth {
    static int launch(ccp_grid *g, const FusedPass &pass)
    {
        if (pass.plan.T == TMAX) return launch_fused_t<TMAX>(g, pass);
        return FusedDepth<TMAX - 1>::launch(g, pass);
    }
    static int launch(ccp_grid *g, const FusedMultiPass &group)
    {
        if (group.first.plan.T == TMAX) return launch_fused_multi_t<TMAX>(g, group);
        return FusedDepth<TMAX - 1>::launch(g, group);
    }
};
template <>
struct FusedDepth<0> {
    static int launch(ccp_grid *, const FusedPass &) { return CCP_ERR_BAD_ARG; }
    static int launch(ccp_grid *, const FusedMultiPass &) { return CCP_ERR_UNSUPPORTED; }
};

// A planned pass / group of passes of any depth: what ccp_grid_tune and the loops below launch through.
int launch_pass(ccp_grid *g, const FusedPass &pass) { return FusedDepth<kFusedMaxT>::launch(g, pass); }
int launch_pass(ccp_grid *g, const FusedMultiPass &group) { return FusedDepth<kFusedMaxT>::launch(g, group); }

// An unchecked pass over every local row, whatever the ghosts hold (ccp_grid_tune times these)
FusedPass whole_block_pass(const ccp_grid *g, int T, const double *xin, double *xout)
{
    FusedPassKind kind;
    kind.T = T;
    kind.st_hi = g->geom.local_rows;
    FusedPass pass = plan_pass(g, kind);
    pass.xin = xin;
    pass.xout = xout;
    return pass;
}

// The group of n passes of depth T whose pass q stores rows [lo[q], hi[q]), from xin to xout and back
FusedMultiPass plan_multi_pass(const ccp_grid *g, int T, int n, const int *lo, const int *hi, const double *xin, double *xout, int red_skip = 0)
{
    FusedMultiPass group;
    FusedPassKind kind;
    kind.T = T;
    kind.st_lo = lo[0];
    kind.st_hi = hi[0];
    kind.multi = true;
    group.first = plan_pass(g, kind);
    group.first.xin = xin;
    group.first.xout = xout;
    group.n_passes = n;
    for (int q = 0; q < kMultiMaxPasses; ++q) {
        group.st_lo[q] = q < n ? lo[q] : 0;
        group.st_hi[q] = q < n ? hi[q] : 0;
    }
    group.red_skip = red_skip;
    return group;
}

__global__ void k_publish_flag(unsigned long long *flag, unsigned long long epoch)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One wave polling the flag (wait_mode 1).  Bounded, so that it cannot hold a hardware queue for ever; a wait
// that gives up is RECORDED in *timed_out (host-mapped) and turns into CCP_ERR_STATE on the host side — what
// follows it on the stream may have sent rows that were not final.
__global__ void k_wait_flag(const unsigned long long *flag, unsigned long long epoch, unsigned long long ticks, unsigned *timed_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
        __builtin_amdgcn_s_sleep(64);
        if (wall_clock64() - t0 > ticks) {                         // 100 MHz constant clock
            __hip_atomic_store(timed_out, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
    }
}

// A new epoch of the edge hand-off: returns the value waiters of THIS pass look for.
void edge_epoch_begin(ccp_grid *g) { g->edge_epoch++; }

// After the pass: whatever happened inside it, the flag reaches the epoch once the whole pass is done
// (also the only publication when the pass could not signal by itself).
int edge_epoch_publish_after_pass(ccp_grid *g)
{
    if (!g->edge_flag) return CCP_OK;
    if (g->wait_mode == 0) {
        CCP_HIP(hipStreamWriteValue64(g->stream, g->edge_flag, g->edge_epoch, 0));      // a queue packet, no kernel launch
    } else {
        hipLaunchKernelGGL(k_publish_flag, dim3(1), dim3(64), 0, g->stream, g->edge_flag, g->edge_epoch);
        CCP_HIP(hipGetLastError());
    }
    return CCP_OK;
}

// Make `s` wait until the edge rows of the last edge pass are final.
int edge_wait_on_stream(ccp_grid *g, hipStream_t s)
{
    if (!g->edge_flag) return CCP_OK;
    if (g->wait_mode == 0) {
        CCP_HIP(hipStreamWaitValue64(s, g->edge_flag, g->edge_epoch, hipStreamWaitValueGte, ~0ull));
    } else {
        hipLaunchKernelGGL(k_wait_flag, dim3(1), dim3(64), 0, s, g->edge_flag, g->edge_epoch, g->edge_timeout_ticks, g->edge_timeout);
        CCP_HIP(hipGetLastError());
    }
    return CCP_OK;
}

// T fused iterations xin -> xout, with the ghost bookkeeping of 2T half-sweeps.
// edge_rows > 0 (row blocks with neighbours): the owned rows next to each neighbour are finished first
// inside the launch and published through the edge flag (see plan_pass); without an in-launch
// signal the flag is published after the pass.  Same tiles, same arithmetic.
int launch_fused(ccp_grid *g, int T, const double *xin, double *xout, const int *active, int l1 = 0,
                 long *l1_blocks = nullptr, int edge_rows = 0, bool store_red = true)
{
    if (T < 1 || T > kFusedMaxT) return CCP_ERR_BAD_ARG;
    const FusedPlanInput in = plan_input(g, T);
    const int s = g->half_sweeps_since_refresh + 2 * T;
    if (fused_ghosts_exhausted(in, s)) return CCP_ERR_STATE;            // refresh first
    FusedPassKind kind;
    kind.T = T;
    kind.l1 = l1;
    fused_stored_rows(in, s, kind.st_lo, kind.st_hi);
    if (kind.st_hi > kind.st_lo) {
        FusedPass pass = plan_pass(g, kind, active, edge_rows);
        pass.xin = xin;
        pass.xout = xout;
        pass.l1_blocks = l1_blocks;
        pass.store_red = store_red || l1 != 0 || edge_rows > 0;
        CCP_TRY(launch_pass(g, pass));
    }
    if (in.stale_top || in.stale_bottom) g->half_sweeps_since_refresh = s;
    return CCP_OK;
}

// x_alt, the ping-pong partner of x, exists from its first use on (cleared once: passes read its pads)
int ensure_x_alt(ccp_grid *g)
{
    if (g->x_alt.p) return CCP_OK;
    const size_t elems = (size_t)g->geom.ch_stride * g->desc.channels;
    CCP_TRY(g->x_alt.alloc(elems));
    CCP_HIP(hipMemsetAsync(g->x_alt.p, 0, elems * sizeof(double), g->stream));
    return CCP_OK;
}

// `iterations` unchecked sweeps: an even number of fused launches (so the result lands back
// in g->x), a lone leftover iteration through the in-place half-sweep kernels.
// l1_last: the last launch also accumulates the L1 step of the final iteration (fused check).
// edge_rows > 0: a new edge epoch — the last launch hands the neighbours' rows over early.
int run_unchecked(ccp_grid *g, int iterations, const int *active = nullptr, bool l1_last = false,
                  long *l1_blocks = nullptr, int edge_rows = 0)
{
    if (edge_rows > 0) edge_epoch_begin(g);
    if (!g->fuse || iterations < 2) {
        if (l1_last) return CCP_ERR_STATE;
        for (int k = 0; k < iterations; ++k) CCP_TRY(one_iteration(g, false, active, nullptr));
        if (edge_rows > 0) CCP_TRY(edge_epoch_publish_after_pass(g));
        return CCP_OK;
    }
    CCP_TRY(ensure_x_alt(g));
    // The passes (fused_pass_split): measured per-depth launch times when the handle was tuned, otherwise "fewer, deeper
    // launches are cheaper"; an odd number of them only where x and x_alt may swap roles.
    double cost[kFusedMaxT + 1] = {0};
    for (int T = 1; T <= kFusedMaxT; ++T) cost[T] = g->tuned && g->tune_ms[T] > 0 ? (double)g->tune_ms[T] : fused_default_cost(T);
    const FusedPassSplit split = fused_pass_split(iterations, g->fuse_tmax, cost, g->allow_swap && !g->ghost_top && !g->ghost_bottom && edge_rows == 0);
    if (split.in_place && l1_last) return CCP_ERR_STATE;
    if (split.depths.empty()) return CCP_ERR_STATE;
    const std::vector<int> &plan = split.depths;
    // the hand-off belongs to the last iteration: a pass hands over only when no in-place iteration follows it
    const int pass_edge_rows = split.in_place ? 0 : edge_rows;
    auto stores_red = [&](size_t k) { return fused_stores_red(k, plan.size(), l1_last, g->red_store_all); };
    double *cur = g->x.p, *alt = g->x_alt.p;
    for (size_t k = 0; k < plan.size();) {
        // consecutive passes of one depth as ONE launch (k_fused_multi), where that is switched on and the shape
        // qualifies; the pass that carries the stop rule or the edge hand-off keeps its own kernels
        if (g->multi && active == nullptr) {
            size_t j = k;
            while (j < plan.size() && plan[j] == plan[k] && (int)(j - k) < kMultiMaxPasses &&
                   !(j + 1 == plan.size() && (l1_last || pass_edge_rows > 0)))
                ++j;
            const int n = (int)(j - k), T = plan[k];
            const FusedPlanInput in = plan_input(g, T);
            const int since = g->half_sweeps_since_refresh;
            if (n >= 2 && !fused_ghosts_exhausted(in, since + 2 * T * n)) {
                int lo[kMultiMaxPasses], hi[kMultiMaxPasses];
                for (int q = 0; q < n; ++q) fused_stored_rows(in, since + 2 * T * (q + 1), lo[q], hi[q]);
                int red_skip = 0;                                 // the leading passes of the group that may skip red
                while (red_skip < n && !stores_red(k + red_skip)) ++red_skip;
                const int st = launch_pass(g, plan_multi_pass(g, T, n, lo, hi, cur, alt, red_skip));
                if (st == CCP_OK) {
                    if (in.stale_top || in.stale_bottom) g->half_sweeps_since_refresh += 2 * T * n;
                    if (n & 1) std::swap(cur, alt);
                    k = j;
                    continue;
                }
                if (st != CCP_ERR_UNSUPPORTED) return st;
            }
        }
        const bool last = k + 1 == plan.size();
        CCP_TRY(launch_fused(g, plan[k], cur, alt, active, (l1_last && last) ? 1 : 0, l1_blocks, last ? pass_edge_rows : 0, stores_red(k)));
        std::swap(cur, alt);
        ++k;
    }
    if (cur != g->x.p) {
        // an odd number of passes (free_parity): the result is in the partner buffer, which becomes x
        if (!split.free_parity) return CCP_ERR_STATE;
        std::swap(g->x.p, g->x_alt.p);
        std::swap(g->x.n, g->x_alt.n);
    }
    for (int k = 0; k < split.in_place; ++k) CCP_TRY(one_iteration(g, false, active, nullptr));
    if (edge_rows > 0) CCP_TRY(edge_epoch_publish_after_pass(g));
    return CCP_OK;
}

// Dirichlet-mask grids: p := 0 wherever the mask byte is 0 (all channels).  grid = (blocks, 1, channels)
__global__ void __launch_bounds__(kBlock)
k_zero_unmasked(double *__restrict__ p, const unsigned char *__restrict__ mask, long per_channel)
{
    double *__restrict__ q = p + (long)blockIdx.z * per_channel;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < per_channel; i += (long)gridDim.x * kBlock)
        if (mask[i] == 0) q[i] = 0.0;
}

}  // namespace

namespace ccp {

int zero_unmasked(ccp_grid *g, double *plane)
{
    if (!g->masked) return CCP_OK;
    hipLaunchKernelGGL(k_zero_unmasked, dim3(2048, 1, (unsigned)g->desc.channels), dim3(kBlock), 0, g->stream, plane, g->maskp.p,
                       g->geom.ch_stride);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int begin_timing(ccp_grid *g)
{
    g->last_launches = 0;
    g->timing_pending = false;
    CCP_HIP(hipEventRecord(g->ev0, g->stream));
    return CCP_OK;
}

int end_timing(ccp_grid *g)
{
    CCP_HIP(hipEventRecord(g->ev1, g->stream));
    g->timing_pending = true;
    return CCP_OK;
}

}  // namespace ccp

namespace {

// ---- Steps the solve entry points share (NOTES.md §R22.1).  The drivers around them stay apart: the one-block loop runs one
// ---- pass ahead of the host, the row-block loop is synchronous, row-block CG fetches ghost rows and all-reduces.

// The step of one checked sweep from its block results (blocks[0/1]: per channel, red / black region) and, with st, the
// stop rule on it; out != nullptr: the sums go there (row blocks all-reduce them)
int launch_check(ccp_grid *g, const long *blocks, double epsilon, int sweep_index, SolveState *st, double *out)
{
    hipLaunchKernelGGL(k_check, dim3((unsigned)g->desc.channels), dim3(kBlock), 0, g->stream, g->partial.p, blocks[0],
                       g->partial.p + g->partial_region, blocks[1], epsilon, sweep_index, st, out);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// What the checked fused passes work in beside x: its partner, the one-channel mask of a re-run, the sums of a pass's sweeps
int ensure_checked_work(ccp_grid *g)
{
    CCP_TRY(ensure_x_alt(g));
    if (!g->redo_mask.p) CCP_TRY(g->redo_mask.alloc(kMaxChannels));
    if (!g->sweep_sums.p) CCP_TRY(g->sweep_sums.alloc((size_t)kFusedMaxCheckedT * kMaxChannels));
    return CCP_OK;
}

// `double eps = 10` (sparse-matrix.h:354), every channel iterating: on the host and (enqueued) on the device
int start_solve_state(ccp_grid *g, SolveState &host)
{
    host = SolveState{};
    for (int ch = 0; ch < g->desc.channels; ++ch) {
        host.active[ch] = 1;
        host.last_eps[ch] = 10.0;
    }
    CCP_HIP(hipMemcpyAsync(g->state.p, &host, sizeof(host), hipMemcpyHostToDevice, g->stream));
    return CCP_OK;
}

// One checked pass of depth T, cur -> alt, over the channels still active: the step of each of its sweeps (a block per
// channel and sweep), reduce(count) on those T * C sums in g->sweep_sums (row blocks: the all-reduce), then the rule on
// them in sweep order (k0 + 1 is the first sweep's index).
template <class Reduce>
int checked_pass(ccp_grid *g, int T, const double *cur, double *alt, int k0, int check_every, double epsilon, Reduce reduce)
{
    const int C = g->desc.channels;
    long blocks[2] = {0, 0};
    CCP_TRY(launch_fused(g, T, cur, alt, reinterpret_cast<const int *>(g->state.p), 2, blocks));
    hipLaunchKernelGGL(k_sweep_sums_wide, dim3((unsigned)C, (unsigned)T), dim3(kBlock), 0, g->stream, g->partial.p, blocks[0],
                       g->partial.p + g->partial_region, blocks[1], g->sweep_sums.p);
    CCP_HIP(hipGetLastError());
    CCP_TRY(reduce((size_t)T * C));
    hipLaunchKernelGGL(k_decide_sums, dim3(1), dim3(kMaxChannels), 0, g->stream, g->sweep_sums.p, C, T, k0 + 1, check_every, epsilon, g->state.p);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// After the host has seen the state behind the pass (k0, T, cur -> alt): a channel that stopped inside it is re-run from
// the pass's input buffer (still intact: passes ping-pong) for exactly the sweeps it wanted, then kept in BOTH buffers — a
// frozen channel is never touched again.  since0: the ghost-row counter when the pass started; the re-run starts there.
int settle_stopped(ccp_grid *g, const SolveState &host, int *was_active, int k0, int T, double *cur, double *alt, int since0, bool *any_active)
{
    const size_t plane = (size_t)g->geom.ch_stride * sizeof(double);
    const int since1 = g->half_sweeps_since_refresh;
    *any_active = false;
    for (int ch = 0; ch < g->desc.channels; ++ch) {
        *any_active |= host.active[ch] != 0;
        if (!was_active[ch] || host.active[ch]) continue;
        was_active[ch] = 0;                                   // stopped inside this pass
        const int m = host.iterations[ch] - k0;               // sweeps of the pass it wanted: 1..T
        double *have = alt;                                   // where the channel's x_k is
        if (m < T) {
            int mask[kMaxChannels] = {0};
            mask[ch] = 1;
            CCP_HIP(hipMemcpyAsync(g->redo_mask.p, mask, sizeof(mask), hipMemcpyHostToDevice, g->stream));
            g->half_sweeps_since_refresh = since0;
            double *p = cur, *q = alt;
            for (int left = m; left > 0;) {
                const int t = std::min(left, g->masked ? kMaskedMaxT : kFusedMaxT);
                CCP_TRY(launch_fused(g, t, p, q, g->redo_mask.p));
                std::swap(p, q);
                left -= t;
            }
            CCP_HIP(hipStreamSynchronize(g->stream));          // `mask` lives on this stack frame
            g->half_sweeps_since_refresh = since1;
            have = p;
        }
        double *other = (have == cur) ? alt : cur;
        CCP_HIP(hipMemcpyAsync(other + (size_t)ch * g->geom.ch_stride, have + (size_t)ch * g->geom.ch_stride, plane,
                               hipMemcpyDeviceToDevice, g->stream));
    }
    return CCP_OK;
}

// Conjugate gradient: the work vectors (one channel each), the loop CCP_GS_CG_FUSED asks for — 0 the three-pass loop
// (88 B), 2 the fused loop with the row-per-block pass A (one block only; its iterates are the three-pass loop's bit for
// bit), otherwise the fused loop with the marching pass A (default) — and the masked / unmasked kernels (launches only: the
// caller asks hipGetLastError its own way, CCP_HIP outside CG and a bare CCP_ERR_HIP in the CG lambdas, as before).
int ensure_cg_work(ccp_grid *g)
{
    if (g->cg_r.p) return CCP_OK;
    const size_t n = (size_t)g->geom.ch_stride;
    CCP_TRY(g->cg_r.alloc(n));
    CCP_TRY(g->cg_p.alloc(n));
    CCP_TRY(g->cg_p2.alloc(n));
    CCP_TRY(g->cg_ap.alloc(n));
    CCP_TRY(g->cg_state.alloc(1));
    return CCP_OK;
}

// k_apply<2, DOT> on rows l_lo + blockIdx.y: out := A in (DOT 0), the residual's sums of in against out (1), out := A in and in'(A in) (2)
template <int DOT>
void launch_apply(ccp_grid *g, dim3 grid, const double *in, double *out, int l_lo)
{
    if (g->masked) hipLaunchKernelGGL((k_apply<2, DOT, true>), grid, dim3(kBlock), 0, g->stream, in, out, out, g->geom, l_lo, g->partial.p, g->maskp.p);
    else hipLaunchKernelGGL((k_apply<2, DOT>), grid, dim3(kBlock), 0, g->stream, in, out, out, g->geom, l_lo, g->partial.p, static_cast<const unsigned char *>(nullptr));
}

// Pass A of the fused loop, marching march_rows rows per block over rows [row_lo, row_hi)
void launch_apply_march(ccp_grid *g, dim3 mgrid, double *xv, const double *rv, const double *p_in, double *p_out, double *apv, int march_rows,
                       int row_lo, int row_hi)
{
    if (g->masked)
        hipLaunchKernelGGL((k_cg_apply_march<true>), mgrid, dim3(kBlock), 0, g->stream, xv, rv, p_in, p_out, apv, g->geom, march_rows, g->partial.p,
                           g->maskp.p, g->cg_state.p, row_lo, row_hi);
    else
        hipLaunchKernelGGL((k_cg_apply_march<false>), mgrid, dim3(kBlock), 0, g->stream, xv, rv, p_in, p_out, apv, g->geom, march_rows, g->partial.p,
                           static_cast<const unsigned char *>(nullptr), g->cg_state.p, row_lo, row_hi);
}

}  // namespace

extern "C" {

int ccp_grid_create(const ccp_grid_desc *d, ccp_grid **out)
try {
    if (!d || !out) return CCP_ERR_BAD_ARG;
    *out = nullptr;
    if (d->width < 1 || d->height < 1 || d->channels < 1 || d->channels > kMaxChannels) return CCP_ERR_BAD_ARG;
    if (d->row_begin < 0 || d->row_count < 1 || d->row_begin + d->row_count > d->height || d->ghost < 0)
        return CCP_ERR_BAD_ARG;
    if ((long)d->width * d->height > 0x7fffffffL) return CCP_ERR_BAD_ARG;   // int32 indices, as the reference
    if ((d->flags & CCP_GRID_WEIGHTED) &&
        ((d->flags & CCP_GRID_DIRICHLET_MASK) || d->ghost != 0 || d->row_begin != 0 || d->row_count != d->height))
        return CCP_ERR_UNSUPPORTED;                                       // weighted grids: single blocks, no mask
    CCP_TRY(select_device(d->device));
    ccp_grid *g = new (std::nothrow) ccp_grid();
    if (!g) return CCP_ERR_ALLOC;
    g->desc = *d;
    g->device = d->device;
    g->ghost_top = d->row_begin > 0 ? std::min(d->ghost, d->row_begin) : 0;
    g->ghost_bottom = (d->row_begin + d->row_count < d->height) ? std::min(d->ghost, d->height - d->row_begin - d->row_count) : 0;
    Geom &geo = g->geom;
    geo.W = d->width;
    geo.H = d->height;
    geo.y0 = d->row_begin - g->ghost_top;
    g->shrink_top = geo.y0 > 0;
    g->shrink_bottom = d->row_begin + d->row_count + g->ghost_bottom < d->height;
    geo.local_rows = g->ghost_top + d->row_count + g->ghost_bottom;
    geo.own_lo = g->ghost_top;
    geo.own_hi = g->ghost_top + d->row_count;
    geo.pitch = (((long)d->width + 1) / 2 + 15) / 16 * 16;
    geo.ch_stride = (long)geo.local_rows * 2 * geo.pitch;
    g->cpt = 2;
    if (const char *e = getenv("CCP_GS_FUSE")) g->fuse = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_SHORT_EDGES")) g->short_edges = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_XCD")) g->xcd_swizzle = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_MULTI")) g->multi = atoi(e);
    if (const char *e = getenv("CCP_GS_TRACE_FILE")) g->trace_file = e[0] ? e : nullptr;
    if (const char *e = getenv("CCP_GS_SIDE_ROWS")) g->side_rows_override = atoi(e);
    if (const char *e = getenv("CCP_GS_LEX_MODE"))
        g->lex_mode = strcmp(e, "planes") == 0 ? 0 : 3;
    if (const char *e = getenv("CCP_GS_TMAX")) g->fuse_tmax = std::max(1, std::min(kFusedMaxT, atoi(e)));
    if (const char *e = getenv("CCP_GS_ALL_BORDER")) g->all_border = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_FORCE_BORDER")) g->force_border = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_RED_STORE")) g->red_store_all = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_WIDE")) g->wide = atoi(e) != 0;
    if (const char *e = getenv("CCP_GS_WIDE_SEGMENTS")) g->wide_segments = std::max(0, atoi(e));
    if (hipDeviceGetAttribute(&g->cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess || g->cus < 1) {
        delete g;
        return CCP_ERR_HIP;
    }
    if (const char *e = getenv("CCP_GS_CHUNK")) g->rows_per_chunk = std::max(1, atoi(e));
    choose_tiling(g);
    g->masked = (d->flags & CCP_GRID_DIRICHLET_MASK) != 0;
    if (g->masked) {
        // (a row block of a masked grid is a masked grid of its own rows plus ghosts: what lies beyond the ghosts is read
        // as zero like everything outside the region, and is as stale as any ghost — the trapezoid argument covers it)
        g->fuse_tmax = std::min(g->fuse_tmax, kMaskedMaxT);
        if (!getenv("CCP_GS_CHUNK")) g->rows_per_chunk = 160;   // what the tuner picks on region canvases of 4-80 M pixels (untuned handles)
    }

    const size_t elems = (size_t)geo.ch_stride * d->channels;
    int st = g->x.alloc(elems);
    if (st == CCP_OK && g->masked) {
        st = g->maskp.alloc((size_t)geo.ch_stride);
        if (st == CCP_OK && hipMemset(g->maskp.p, 0, (size_t)geo.ch_stride) != hipSuccess) st = CCP_ERR_HIP;
        if (st == CCP_OK) st = g->mask_edge.alloc(2 * (size_t)d->width);
        if (st == CCP_OK && hipMemset(g->mask_edge.p, 0, 2 * (size_t)d->width) != hipSuccess) st = CCP_ERR_HIP;
        if (st == CCP_OK) st = g->mask_counters.alloc(2);
    }
    if (st == CCP_OK) st = g->b.alloc(elems);
    g->weighted = (d->flags & CCP_GRID_WEIGHTED) != 0;
    if (st == CCP_OK && g->weighted) {
        st = g->wop.alloc(4 * (size_t)geo.ch_stride);
        if (st == CCP_OK && hipMemset(g->wop.p, 0, 4 * sizeof(double) * (size_t)geo.ch_stride) != hipSuccess) st = CCP_ERR_HIP;
        if (st == CCP_OK) st = g->wpart.alloc(4 * (size_t)d->channels * kWeightedApplyBlocks);
        if (st == CCP_OK) st = g->wcount.alloc(1 + 3 * kMaxChannels);
        if (st == CCP_OK) st = g->rcount.alloc(kRefreshCounts);
        if (st == CCP_OK) st = g->op_status.alloc(1);
        if (st == CCP_OK && hipMemset(g->op_status.p, 0, sizeof(unsigned)) != hipSuccess) st = CCP_ERR_HIP;   // no refresh yet: good
    }
    // partial sums: the finest launch is one block per (x tile, row, channel*2) with 2 doubles
    const size_t part = (size_t)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)) * geo.local_rows * d->channels * 2 * 2 + 64;
    g->partial_region = (long)(part / 2);
    if (st == CCP_OK) st = g->partial.alloc(part);
    if (st == CCP_OK) st = g->small.alloc(4 * kMaxChannels);
    if (st == CCP_OK) st = g->io_bad.alloc(1);
    if (st == CCP_OK) st = g->state.alloc(1);
    g->stage_rows = std::max<long>(1, std::min<long>(geo.local_rows, (8L << 20) / d->width));
    if (st == CCP_OK) st = g->stage.alloc((size_t)g->stage_rows * d->width);
    if (st == CCP_OK && (hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess)) st = CCP_ERR_HIP;
    if (st == CCP_OK && (hipStreamCreateWithFlags(&g->stream2, hipStreamNonBlocking) != hipSuccess ||
                         hipEventCreateWithFlags(&g->ev_main, hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&g->ev_side, hipEventDisableTiming) != hipSuccess))
        st = CCP_ERR_HIP;
    if (st == CCP_OK && (g->ghost_top || g->ghost_bottom)) {
        // edge hand-off of a row block with neighbours: counter in device memory, flag in signal memory
        int can_wait = 0;
        (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, g->device);
        g->wait_mode = can_wait ? 0 : 1;
        if (const char *e = getenv("CCP_GS_EDGE_WAIT")) g->wait_mode = (strcmp(e, "spin") == 0) ? 1 : (can_wait ? 0 : 1);
        if (const char *e = getenv("CCP_GS_EDGE_SIGNAL")) g->edge_signal = atoi(e) != 0;
        if (hipMalloc(reinterpret_cast<void **>(&g->edge_counter), sizeof(unsigned long long) * kEdgeRing) != hipSuccess ||
            hipExtMallocWithFlags(reinterpret_cast<void **>(&g->edge_flag), sizeof(unsigned long long), hipMallocSignalMemory) != hipSuccess ||
            hipMemset(g->edge_counter, 0, sizeof(unsigned long long) * kEdgeRing) != hipSuccess ||
            hipMemset(g->edge_flag, 0, sizeof(unsigned long long)) != hipSuccess)
            st = CCP_ERR_HIP;
        if (const char *e = getenv("CCP_GS_EDGE_TIMEOUT_TICKS")) g->edge_timeout_ticks = strtoull(e, nullptr, 10);
    }
    // the word in which a kernel records a bounded wait that gave up (k_wait_flag, k_fused_multi): host-mapped
    if (st == CCP_OK && hipHostMalloc(reinterpret_cast<void **>(&g->edge_timeout), sizeof(unsigned), hipHostMallocMapped) != hipSuccess) st = CCP_ERR_HIP;
    if (g->edge_timeout) *g->edge_timeout = 0;
    if (st == CCP_OK && (hipMemset(g->x.p, 0, elems * sizeof(double)) != hipSuccess ||
                         hipMemset(g->b.p, 0, elems * sizeof(double)) != hipSuccess))
        st = CCP_ERR_HIP;
    if (st != CCP_OK) {
        ccp_grid_destroy(g);
        return st;
    }
    *out = g;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_destroy(ccp_grid *g)
try {
    if (!g) return CCP_OK;
    (void)hipSetDevice(g->device);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->ev_r0) (void)hipEventDestroy(g->ev_r0);
    if (g->ev_r1) (void)hipEventDestroy(g->ev_r1);
    if (g->ev_main) (void)hipEventDestroy(g->ev_main);
    if (g->ev_side) (void)hipEventDestroy(g->ev_side);
    if (g->stream2) {
        (void)hipStreamSynchronize(g->stream2);
        (void)hipStreamDestroy(g->stream2);
    }
    if (g->stream_comm) {
        (void)hipStreamSynchronize(g->stream_comm);
        (void)hipStreamDestroy(g->stream_comm);
    }
    if (g->ev_comm) (void)hipEventDestroy(g->ev_comm);
    if (g->ev_ready) (void)hipEventDestroy(g->ev_ready);
    if (g->edge_counter) (void)hipFree(g->edge_counter);
    if (g->edge_flag) (void)hipFree(g->edge_flag);
    if (g->edge_timeout) (void)hipHostFree(g->edge_timeout);
    if (g->lex_order_pin) (void)hipHostFree(g->lex_order_pin);
    mg_release(&g->mg);
    delete g;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_get_layout(ccp_grid *g, ccp_grid_layout *out)
try {
    if (!g || !out) return CCP_ERR_BAD_ARG;
    out->x_dev = g->x.p;
    out->b_dev = g->b.p;
    out->pitch = g->geom.pitch;
    out->local_rows = g->geom.local_rows;
    out->ghost_top = g->ghost_top;
    out->ghost_bottom = g->ghost_bottom;
    out->channels = g->desc.channels;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_stream(ccp_grid *g, void *hip_stream)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    g->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_synchronize(ccp_grid *g)
try {
    CCP_TRY(bind(g));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return edge_timeout_status(g);
} CCP_ABI_CATCH

}  // extern "C"

// Library-internal: what ccp_grid_mg.hip needs of a handle
int ccp::grid_mg_view(ccp_grid *g, GridMgView *v)
{
    CCP_TRY(bind(g));
    v->geom = g->geom;
    v->channels = g->desc.channels;
    v->masked = g->masked;
    v->one_block = !g->ghost_top && !g->ghost_bottom && g->desc.row_count == g->desc.height;
    v->x = g->x.p;
    v->b = g->b.p;
    v->mask = g->maskp.p;
    v->weighted = g->weighted;
    const double *op = g->weighted && g->has_op ? g->wop.p : nullptr;
    const long n = g->geom.ch_stride;
    v->wd = op;
    v->wwe = op ? op + n : nullptr;
    v->wws = op ? op + 2 * n : nullptr;
    v->wlam = !op ? nullptr : g->has_fixed ? g->wcons.p + 2 * n : op + 3 * n;   // with fixed pixels: lambda' (ccp_grid_weighted.hpp)
    v->op_channels = g->weighted && g->has_op && g->per_channel ? g->desc.channels : 1;
    v->op_stride = 4 * n;
    v->lam_stride = g->has_fixed ? 3 * n : 4 * n;
    v->cfg = g->mg_cfg;
    v->ns = &g->mg_nullspace;
    v->refreshed = g->refreshed;
    v->op_status = g->op_status.p;
    v->op_verdict = g->rcount.p;
    v->stream = g->stream;
    v->device = g->device;
    v->cache = &g->mg;
    v->comm = g->comm;
    v->part = g->part.empty() ? nullptr : g->part.data();
    v->ghost = g->desc.ghost;
    return CCP_OK;
}

int ccp::grid_mg_slot(ccp_grid *g, GridMgSlot *s)
{
    CCP_TRY(bind(g));
    s->cfg = &g->mg_cfg;
    s->cache = &g->mg;
    s->weighted = g->weighted;
    s->row_block = g->desc.ghost != 0 || g->desc.row_count < g->desc.height;
    return CCP_OK;
}

void ccp::grid_mg_halo_stale(ccp_grid *g) { g->half_sweeps_since_refresh = g->desc.ghost; }

int ccp::grid_set_allow_swap(ccp_grid *g, bool on)
{
    if (!g) return CCP_ERR_BAD_ARG;
    g->allow_swap = on;
    return CCP_OK;
}

extern "C" {

int ccp_grid_fill_x(ccp_grid *g, double value)
try {
    CCP_TRY(bind(g));
    const long n = g->geom.ch_stride * g->desc.channels;
    hipLaunchKernelGGL(k_fill, dim3(2048), dim3(kBlock), 0, g->stream, g->x.p, n, value);
    CCP_HIP(hipGetLastError());
    CCP_TRY(zero_unmasked(g, g->x.p));
    g->half_sweeps_since_refresh = 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_randomize_x(ccp_grid *g, uint64_t seed, double lo, double hi)
try {
    CCP_TRY(bind(g));
    dim3 grid((unsigned)((g->geom.pitch + kBlock - 1) / kBlock), (unsigned)g->geom.local_rows, (unsigned)g->desc.channels * 2);
    hipLaunchKernelGGL(k_randomize, grid, dim3(kBlock), 0, g->stream, g->x.p, g->geom, seed, lo, hi);
    CCP_HIP(hipGetLastError());
    CCP_TRY(zero_unmasked(g, g->x.p));
    g->half_sweeps_since_refresh = 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_b_from_x(ccp_grid *g)
try {
    CCP_TRY(bind(g));
    if (g->weighted) {
        if (!g->has_op) return CCP_ERR_STATE;
        return weighted_apply(g, 0);
    }
    if ((g->shrink_top || g->shrink_bottom) && g->half_sweeps_since_refresh >= g->desc.ghost) return CCP_ERR_STATE;
    const Geom &geo = g->geom;
    // every local row whose neighbour rows are local too: the ghost rows need their b as well
    // (they are recomputed between halo exchanges); only the outermost ghost row cannot get one
    const int l_lo = g->shrink_top ? 1 : 0;
    const int l_hi = geo.local_rows - (g->shrink_bottom ? 1 : 0);
    dim3 grid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)(l_hi - l_lo), (unsigned)g->desc.channels * 2);
    launch_apply<0>(g, grid, g->x.p, g->b.p, l_lo);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_halo_refreshed(ccp_grid *g)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    g->half_sweeps_since_refresh = 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_sweep(ccp_grid *g, int32_t iterations)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (iterations < 0) return CCP_ERR_BAD_ARG;
    CCP_TRY(begin_timing(g));
    CCP_TRY(run_unchecked(g, iterations));
    CCP_TRY(end_timing(g));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_sweep_edges_first(ccp_grid *g, int32_t iterations, int32_t edge_rows)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (iterations < 0 || edge_rows < 0) return CCP_ERR_BAD_ARG;
    if (!g->edge_flag) return ccp_grid_sweep(g, iterations);          // no neighbour blocks: nothing to hand over early
    CCP_TRY(begin_timing(g));
    CCP_TRY(run_unchecked(g, iterations, nullptr, false, nullptr, std::max(1, edge_rows)));
    CCP_TRY(end_timing(g));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_stream_wait_edges(ccp_grid *g, void *hip_stream)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    return edge_wait_on_stream(g, reinterpret_cast<hipStream_t>(hip_stream));
} CCP_ABI_CATCH

int ccp_grid_tune(ccp_grid *g, int32_t max_t, int32_t *chosen_t, int32_t *chosen_rows_per_chunk, float *ms_per_iteration)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (max_t < 1) return CCP_ERR_BAD_ARG;
    max_t = std::min<int>(max_t, g->masked ? kMaskedMaxT : kFusedMaxT);
    CCP_TRY(ensure_x_alt(g));
    const int saved_chunk = g->rows_per_chunk, saved_launches = g->last_launches;
    const bool saved_tuned = g->tuned;
    g->tuned = false;                                  // candidates below set rows_per_chunk directly
    float tab_ms[kFusedMaxT + 1] = {0};
    int tab_rows[kFusedMaxT + 1] = {0};
    const int rows = g->geom.local_rows;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device);
    float best = 1e30f;
    int best_t = 1, best_r = saved_chunk;
    hipEvent_t e0, e1;
    CCP_HIP(hipEventCreate(&e0));
    CCP_HIP(hipEventCreate(&e1));
    int status = CCP_OK;
    for (int T = 1; T <= max_t && status == CCP_OK; ++T) {
        const long slots = (long)cus * (g->masked ? masked_waves_per_simd(T) : fused_waves_per_simd(T));       // resident workgroups
        const std::vector<int> chunk_candidates = fused_tune_chunk_rows(g->geom, g->desc.channels, T, slots);
        for (int R : chunk_candidates) {
            if (R > rows && R != chunk_candidates[0]) continue;
            g->rows_per_chunk = R;
            auto once = [&]() -> int { return launch_pass(g, whole_block_pass(g, T, g->x.p, g->x_alt.p)); };
            status = once();                                   // warm (code, TLB)
            if (status != CCP_OK) break;
            (void)hipEventRecord(e0, g->stream);
            status = once();
            if (status == CCP_OK) status = once();
            (void)hipEventRecord(e1, g->stream);
            if (status != CCP_OK) break;
            if (hipEventSynchronize(e1) != hipSuccess) { status = CCP_ERR_HIP; break; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            const float per_launch = ms / 2.0f;
            if (getenv("CCP_GS_DEBUG"))
                fprintf(stderr, "[ccp_gs] tune T=%d rows/chunk=%d: %.4f ms/launch, %.5f ms/iteration\n", T, R, per_launch, per_launch / T);
            if (tab_ms[T] == 0.f || per_launch < tab_ms[T]) {
                tab_ms[T] = per_launch;
                tab_rows[T] = R;
            }
            const float per_iter = per_launch / T;
            if (per_iter < best) {
                best = per_iter;
                best_t = T;
                best_r = R;
            }
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    g->last_launches = saved_launches;
    g->rows_per_chunk = saved_chunk;
    if (status != CCP_OK) {
        g->tuned = saved_tuned;
        return status;
    }
    for (int T = 1; T <= kFusedMaxT; ++T) {
        g->tune_ms[T] = tab_ms[T];
        g->tune_rows[T] = tab_rows[T];
    }
    g->tuned = true;
    g->fuse_tmax = max_t;
    // Several passes in ONE launch (k_fused_multi) pay where a pass is short against the drain and fill between two
    // dependent launches: +5 % at 4096^2 x 3, nothing at 16384^2 (NOTES.md).  Decided here by timing four passes of the
    // chosen depth both ways on this shape (whole-image handles; CCP_GS_MULTI overrides).  x is put back afterwards.
    if (!getenv("CCP_GS_MULTI") && !g->shrink_top && !g->shrink_bottom && !g->trace_file && best_t >= 2) {
        const size_t elems = (size_t)g->geom.ch_stride * g->desc.channels;
        DevBuf<double> keep;
        if (keep.alloc(elems) == CCP_OK) {
            CCP_HIP(hipMemcpyAsync(keep.p, g->x.p, elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
            hipEvent_t t0, t1, t2;
            CCP_HIP(hipEventCreate(&t0));
            CCP_HIP(hipEventCreate(&t1));
            CCP_HIP(hipEventCreate(&t2));
            int lo[kMultiMaxPasses], hi[kMultiMaxPasses];
            for (int q = 0; q < kMultiMaxPasses; ++q) {
                lo[q] = 0;
                hi[q] = rows;
            }
            int st = CCP_OK;
            auto singles = [&]() {
                for (int q = 0; q < 4 && st == CCP_OK; ++q)
                    st = launch_pass(g, whole_block_pass(g, best_t, (q & 1) ? g->x_alt.p : g->x.p, (q & 1) ? g->x.p : g->x_alt.p));
            };
            auto multi = [&]() { if (st == CCP_OK) st = launch_pass(g, plan_multi_pass(g, best_t, 4, lo, hi, g->x.p, g->x_alt.p)); };
            singles();                                          // warm both
            multi();
            (void)hipEventRecord(t0, g->stream);
            singles();
            singles();
            (void)hipEventRecord(t1, g->stream);
            multi();
            multi();
            (void)hipEventRecord(t2, g->stream);
            float ms_single = 0.f, ms_multi = 0.f;
            if (st == CCP_OK && hipEventSynchronize(t2) == hipSuccess) {
                (void)hipEventElapsedTime(&ms_single, t0, t1);
                (void)hipEventElapsedTime(&ms_multi, t1, t2);
                g->multi = ms_multi < 0.98f * ms_single ? 1 : 0;
                if (getenv("CCP_GS_DEBUG"))
                    fprintf(stderr, "[ccp_gs] tune: 8 passes of depth %d one by one %.3f ms, four per launch %.3f ms -> %s\n", best_t, ms_single, ms_multi,
                            g->multi ? "several passes per launch" : "one pass per launch");
            }
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
            (void)hipEventDestroy(t2);
            CCP_HIP(hipMemcpyAsync(g->x.p, keep.p, elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
            CCP_HIP(hipStreamSynchronize(g->stream));
            g->last_launches = saved_launches;
            if (st != CCP_OK && st != CCP_ERR_UNSUPPORTED) return st;
        }
    }
    if (chosen_t) *chosen_t = best_t;
    if (chosen_rows_per_chunk) *chosen_rows_per_chunk = best_r;
    if (ms_per_iteration) *ms_per_iteration = best;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_fused(ccp_grid *g, int32_t on)
try {
    CCP_TRY(not_weighted(g));
    if (!g) return CCP_ERR_BAD_ARG;
    g->fuse = on != 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_tiling(ccp_grid *g, int32_t max_t, int32_t rows_per_chunk)
try {
    CCP_TRY(not_weighted(g));
    if (!g || max_t < 1 || rows_per_chunk < 2) return CCP_ERR_BAD_ARG;
    g->fuse_tmax = std::min<int>(max_t, kFusedMaxT);
    g->rows_per_chunk = rows_per_chunk + (rows_per_chunk & 1);       // the march advances two rows per trip
    g->tuned = false;                                                // a tuning table would override the request
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_get_tiling(ccp_grid *g, int32_t *max_t, int32_t *rows_per_chunk, int32_t *tuned)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    const int T = g->fuse_tmax;
    if (max_t) *max_t = T;
    if (rows_per_chunk) *rows_per_chunk = (g->tuned && g->tune_rows[T] > 0) ? g->tune_rows[T] : g->rows_per_chunk;
    if (tuned) *tuned = g->tuned ? 1 : 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_sweep_l1(ccp_grid *g, double *l1_per_channel)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!l1_per_channel) return CCP_ERR_BAD_ARG;
    const int C = g->desc.channels;
    CCP_TRY(begin_timing(g));
    long blocks[2] = {0, 0};
    CCP_TRY(one_iteration(g, true, nullptr, blocks));
    CCP_TRY(launch_check(g, blocks, 0.0, 0, nullptr, g->small.p));
    CCP_TRY(end_timing(g));
    CCP_HIP(hipMemcpyAsync(l1_per_channel, g->small.p, sizeof(double) * C, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_gauss_seidel(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t check_every, ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (g->ghost_top || g->ghost_bottom) return CCP_ERR_STATE;   // row blocks are driven by the caller (halo exchange)
    if (check_every < 0) return CCP_ERR_BAD_ARG;
    const int C = g->desc.channels;
    SolveState host;
    CCP_TRY(start_solve_state(g, host));
    CCP_HIP(hipStreamSynchronize(g->stream));   // the upload read a stack variable; and nothing older runs into the timing
    CCP_TRY(begin_timing(g));
    int issued = 0;
    // `while (eps > epsilon && cnt < max_iteration)`: eps starts at 10
    const bool enter = (10.0 > epsilon);
    bool any_active = enter && max_iteration > 0;
    const int *active = reinterpret_cast<const int *>(g->state.p);
    if (any_active && check_every == 0) {
        // fixed count, no stop test: the temporally blocked sweep
        CCP_TRY(run_unchecked(g, max_iteration, nullptr));
        issued = max_iteration;
        any_active = false;
    }
    if (any_active && check_every >= 1 && g->fuse) {
        // The reference tests its stop rule after EVERY sweep (check_every = 1; k > 1 tests every k-th
        // sweep with the same machinery).  A temporally blocked pass knows the
        // previous level of every pixel it updates, so it reports the step of each of its T sweeps
        // (L1 = 2) at no extra traffic; k_decide_sums finds the first sweep that meets the rule.  If
        // that sweep is inside the pass, the channel is re-run from the pass's input buffer (still
        // intact: passes ping-pong) for exactly the missing sweeps — once per solve.
        const size_t elems = (size_t)g->geom.ch_stride * C;
        CCP_TRY(ensure_checked_work(g));
        double *cur = g->x.p, *alt = g->x_alt.p;
        int was_active[kMaxChannels];
        for (int ch = 0; ch < C; ++ch) was_active[ch] = 1;
        // The host runs ONE PASS AHEAD of what it has looked at: pass n+1 is queued before the state after pass n is read
        // back, so the chip does not idle through a host round trip per pass (a pass of 4096^2 x 3 takes 0.3 ms; the
        // round trip was a tenth of it).  That is safe because the rule is applied on the device, in stream order: a
        // channel that stops in pass n is frozen before pass n+1 starts, which then leaves it — and its buffers — alone.
        struct Queued {
            SolveState st;
            int k0 = 0, T = 0;
            double *cur = nullptr, *alt = nullptr;     // the pass read cur and wrote alt
            hipEvent_t ev = nullptr;
        } ring[2];
        for (Queued &q : ring) CCP_HIP(hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
        int k0 = 0, n_queued = 0, n_seen = 0, status = CCP_OK;
        auto queue_pass = [&]() -> int {
            Queued &q = ring[n_queued & 1];
            q.k0 = k0;
            q.T = std::min(g->masked ? kMaskedMaxCheckedT : kFusedMaxCheckedT, max_iteration - k0);
            q.cur = cur;
            q.alt = alt;
            CCP_TRY(checked_pass(g, q.T, cur, alt, k0, check_every, epsilon, [](size_t) { return CCP_OK; }));   // one block: its sums are the sums
            CCP_HIP(hipMemcpyAsync(&q.st, g->state.p, sizeof(q.st), hipMemcpyDeviceToHost, g->stream));
            CCP_HIP(hipEventRecord(q.ev, g->stream));
            k0 += q.T;
            std::swap(cur, alt);
            ++n_queued;
            return CCP_OK;
        };
        auto look_at_pass = [&]() -> int {
            Queued &q = ring[n_seen & 1];
            CCP_HIP(hipEventSynchronize(q.ev));
            host = q.st;
            // (no ghost rows on this handle: the ghost-row counter never moves)
            CCP_TRY(settle_stopped(g, host, was_active, q.k0, q.T, q.cur, q.alt, g->half_sweeps_since_refresh, &any_active));
            ++n_seen;
            return CCP_OK;
        };
        while (status == CCP_OK && any_active && (n_seen < n_queued || k0 < max_iteration)) {
            // keep two passes queued while there are sweeps left, then look at the older one
            while (status == CCP_OK && n_queued - n_seen < 2 && k0 < max_iteration) status = queue_pass();
            if (status == CCP_OK) status = look_at_pass();
        }
        // (passes queued beyond the one that stopped the last channel find every channel frozen: they leave at once)
        if (n_seen < n_queued) (void)hipStreamSynchronize(g->stream);      // (a copy into `ring` may still be in flight)
        for (Queued &q : ring) (void)hipEventDestroy(q.ev);
        CCP_TRY(status);
        if (cur != g->x.p)
            CCP_HIP(hipMemcpyAsync(g->x.p, cur, elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        issued = k0;
        any_active = false;
    }
    const int batch_checks = 8;             // checked sweeps enqueued between two host polls
    while (any_active && issued < max_iteration) {
        int checks = 0;
        while (issued < max_iteration && checks < batch_checks) {
            if (g->fuse && check_every >= 2 && max_iteration - issued >= check_every) {
                // a whole check period in fused launches; the last one accumulates the L1 step of
                // the period's final sweep, so checking costs no extra pass over the grid
                long blocks[2] = {0, 0};
                CCP_TRY(run_unchecked(g, check_every, active, true, blocks));
                issued += check_every;
                CCP_TRY(launch_check(g, blocks, epsilon, issued, g->state.p, nullptr));
                ++checks;
                continue;
            }
            // check_every-1 unchecked sweeps (fused), then one sweep that accumulates the L1 step
            const int plain = std::min(check_every - 1, max_iteration - issued);
            if (plain > 0) {
                CCP_TRY(run_unchecked(g, plain, active));
                issued += plain;
            }
            if (issued >= max_iteration) break;
            long blocks[2] = {0, 0};
            CCP_TRY(one_iteration(g, true, active, blocks));
            ++issued;
            CCP_TRY(launch_check(g, blocks, epsilon, issued, g->state.p, nullptr));
            ++checks;
        }
        CCP_HIP(hipMemcpyAsync(&host, g->state.p, sizeof(host), hipMemcpyDeviceToHost, g->stream));
        CCP_HIP(hipStreamSynchronize(g->stream));
        any_active = false;
        for (int ch = 0; ch < C; ++ch) any_active |= host.active[ch] != 0;
    }
    return finish_solve(g, report, [&](int ch, ccp_gs_report &r) {
        r.converged = host.converged[ch];
        r.iterations = host.converged[ch] ? host.iterations[ch] : issued;
        r.last_l1_step = host.last_eps[ch];
    }, &host);
} CCP_ABI_CATCH

int ccp_grid_conjugate_gradient(ccp_grid *g, double epsilon, int32_t max_iteration, ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (g->ghost_top || g->ghost_bottom || g->desc.row_count != g->desc.height) return CCP_ERR_STATE;
    const Geom &geo = g->geom;
    const long n = geo.ch_stride;                       // one channel incl. pads (pads stay 0 in b, r, p, Ap)
    CCP_TRY(ensure_cg_work(g));
    hipStream_t s = g->stream;
    dim3 grid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)geo.local_rows, 2);
    for (int ch = 0; ch < g->desc.channels; ++ch) {
        CCP_HIP(hipMemsetAsync(g->cg_r.p, 0, sizeof(double) * n, s));
        CCP_HIP(hipMemsetAsync(g->cg_ap.p, 0, sizeof(double) * n, s));
        // matrix-free A*v on one channel: the kernel sees channel 0 of the offset pointers
        auto spmv = [&](const double *in, double *out) -> int {
            launch_apply<0>(g, grid, in, out, 0);
            return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
        };
        auto spmv_dot = [&](const double *in, double *out, int *n_partials) -> int {
            *n_partials = (int)(grid.x * grid.y * grid.z);
            launch_apply<2>(g, grid, in, out, 0);
            return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
        };
        const int fused_mode = cg_fused_mode();
        if (fused_mode == 0) {
            CCP_TRY(cg_solve(spmv, spmv_dot, g->b.p + (long)ch * n, g->x.p + (long)ch * n, g->cg_r.p, g->cg_p.p, g->cg_ap.p, n, epsilon,
                             max_iteration, g->cg_state.p, g->partial.p, s, g->ev0, g->ev1, report ? report + ch : nullptr));
            continue;
        }
        // fused loop: 72 B per unknown and iteration (ccp_cg.hpp); same iterates bit for bit
        CCP_HIP(hipMemsetAsync(g->cg_p2.p, 0, sizeof(double) * n, s));
        const int march_rows = 32;
        const dim3 mgrid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)((geo.local_rows + march_rows - 1) / march_rows));
        auto apply = [&](double *xv, const double *rv, const double *p_in, double *p_out, double *apv, int *n_partials) -> int {
            if (fused_mode != 2) {
                *n_partials = (int)(mgrid.x * mgrid.y);
                launch_apply_march(g, mgrid, xv, rv, p_in, p_out, apv, march_rows, 0, geo.local_rows);
                return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
            }
            if (g->masked)
                hipLaunchKernelGGL((k_cg_apply_fused<2, true>), grid, dim3(kBlock), 0, s, xv, rv, p_in, p_out, apv, geo, g->partial.p, g->maskp.p, g->cg_state.p);
            else
                hipLaunchKernelGGL((k_cg_apply_fused<2, false>), grid, dim3(kBlock), 0, s, xv, rv, p_in, p_out, apv, geo, g->partial.p,
                                   static_cast<const unsigned char *>(nullptr), g->cg_state.p);
            *n_partials = (int)(grid.x * grid.y * grid.z);
            return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
        };
        CCP_TRY(cg_solve_fused(spmv, apply, g->b.p + (long)ch * n, g->x.p + (long)ch * n, g->cg_r.p, g->cg_p.p, g->cg_p2.p, g->cg_ap.p, n,
                               epsilon, max_iteration, g->cg_state.p, g->partial.p, s, g->ev0, g->ev1, report ? report + ch : nullptr));
    }
    return CCP_OK;
} CCP_ABI_CATCH

namespace {

// g->small.p[2*ch] = sum (b - A x)^2, [2*ch+1] = sum b^2 over the OWNED rows (device, on g->stream)
int residual_to_small(ccp_grid *g)
{
    const int C = g->desc.channels;
    if (g->weighted) {
        if (!g->has_op) return CCP_ERR_STATE;
        const dim3 wg = weighted_apply_grid(g);
        CCP_TRY(weighted_apply(g, 1));
        hipLaunchKernelGGL(k_pair_reduce, dim3((unsigned)C), dim3(kBlock), 0, g->stream, g->wpart.p, (long)wg.x, g->small.p);
        CCP_HIP(hipGetLastError());
        return CCP_OK;
    }
    if ((g->shrink_top || g->shrink_bottom) && g->half_sweeps_since_refresh >= g->desc.ghost) return CCP_ERR_STATE;
    const Geom &geo = g->geom;
    dim3 grid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)(geo.own_hi - geo.own_lo), (unsigned)C * 2);
    launch_apply<1>(g, grid, g->x.p, g->b.p, geo.own_lo);
    CCP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pair_reduce, dim3((unsigned)C), dim3(kBlock), 0, g->stream, g->partial.p, (long)grid.x * grid.y, g->small.p);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int small_to_rr_bb(ccp_grid *g, double *rr_bb)
{
    const int C = g->desc.channels;
    double host[2 * kMaxChannels];
    CCP_HIP(hipMemcpyAsync(host, g->small.p, sizeof(double) * 2 * C, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    for (int ch = 0; ch < C; ++ch) {
        rr_bb[ch] = host[2 * ch];
        rr_bb[C + ch] = host[2 * ch + 1];
    }
    return edge_timeout_status(g);
}

}  // namespace

int ccp_grid_residual_norm2(ccp_grid *g, double *rr_bb)
try {
    CCP_TRY(bind(g));
    if (!rr_bb) return CCP_ERR_BAD_ARG;
    CCP_TRY(residual_to_small(g));
    return small_to_rr_bb(g, rr_bb);
} CCP_ABI_CATCH

int ccp_grid_abs_sum(ccp_grid *g, double *per_channel)
try {
    CCP_TRY(bind(g));
    if (!per_channel) return CCP_ERR_BAD_ARG;
    const int C = g->desc.channels;
    const unsigned blocks = 1024;
    hipLaunchKernelGGL(k_abs_sum, dim3(blocks, 1, (unsigned)C), dim3(kBlock), 0, g->stream, g->x.p, g->geom, g->partial.p);
    CCP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sum_reduce, dim3((unsigned)C), dim3(kBlock), 0, g->stream, g->partial.p, (long)blocks, g->small.p);
    CCP_HIP(hipGetLastError());
    CCP_HIP(hipMemcpyAsync(per_channel, g->small.p, sizeof(double) * C, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return edge_timeout_status(g);
} CCP_ABI_CATCH

// ============================================================================================
// Row blocks over RCCL: neighbour halo exchange and all-reduced norms behind the C ABI.
// ============================================================================================
namespace {

bool has_neighbours(const ccp_grid *g) { return g->up_rank >= 0 || g->down_rank >= 0; }

// The messages of one exchange, all in one RCCL group on `s`: the outermost owned rows go to the
// neighbours' ghost rows, theirs arrive in ours.  One image row of one channel is 2*pitch contiguous
// doubles, so a block of rows is one message per channel and direction.
int issue_exchange(ccp_grid *g, hipStream_t s, double *base = nullptr)
{
    const RcclApi *api = rccl_api();
    if (!api || !g->comm) return CCP_ERR_STATE;
    const Geom &geo = g->geom;
    const size_t row = (size_t)2 * geo.pitch;
    if (!base) base = g->x.p;                        // (a checked solve exchanges the buffer its iterate is in)
    CCP_RCCL(api->GroupStart());
    ncclResult_t r = ncclSuccess;
    for (int ch = 0; ch < g->desc.channels && r == ncclSuccess; ++ch) {
        double *x = base + (size_t)ch * geo.ch_stride;
        if (g->up_rank >= 0) {
            r = api->Send(x + (size_t)geo.own_lo * row, (size_t)g->send_up * row, ncclDouble, g->up_rank, g->comm->comm, s);
            if (r == ncclSuccess) r = api->Recv(x, (size_t)g->ghost_top * row, ncclDouble, g->up_rank, g->comm->comm, s);
        }
        if (g->down_rank >= 0 && r == ncclSuccess) {
            r = api->Send(x + (size_t)(geo.own_hi - g->send_down) * row, (size_t)g->send_down * row, ncclDouble, g->down_rank,
                          g->comm->comm, s);
            if (r == ncclSuccess) r = api->Recv(x + (size_t)geo.own_hi * row, (size_t)g->ghost_bottom * row, ncclDouble, g->down_rank,
                                               g->comm->comm, s);
        }
    }
    const ncclResult_t e = api->GroupEnd();
    if (r != ncclSuccess) return rccl_fail(r, "ncclSend/ncclRecv", __FILE__, __LINE__);
    CCP_RCCL(e);
    return CCP_OK;
}

// Refresh the ghost rows.  after_edges: the sweeps were issued with an edge epoch — the messages wait for
// the edge flag only and travel beside the rest of the pass; otherwise they wait for everything queued.
int exchange(ccp_grid *g, bool after_edges, double *base = nullptr)
{
    if (!g->comm) return CCP_ERR_STATE;
    if (has_neighbours(g)) {
        if (after_edges) {
            CCP_TRY(edge_wait_on_stream(g, g->stream_comm));
        } else {
            CCP_HIP(hipEventRecord(g->ev_ready, g->stream));
            CCP_HIP(hipStreamWaitEvent(g->stream_comm, g->ev_ready, 0));
        }
        CCP_TRY(issue_exchange(g, g->stream_comm, base));
        CCP_HIP(hipEventRecord(g->ev_comm, g->stream_comm));
        CCP_HIP(hipStreamWaitEvent(g->stream, g->ev_comm, 0));
        g->exchanges++;
    }
    g->half_sweeps_since_refresh = 0;
    return CCP_OK;
}

// `iterations` sweeps with a halo exchange every ghost/2 iterations.
int sweep_rowblocked(ccp_grid *g, int iterations)
{
    const bool nb = has_neighbours(g);
    const int ipe = std::max(1, g->desc.ghost / 2);
    int left = iterations;
    while (left > 0) {
        int since = g->half_sweeps_since_refresh / 2;
        if (nb && since >= ipe) {
            CCP_TRY(exchange(g, false));
            since = 0;
        }
        const int room = nb ? std::min(left, ipe - since) : left;
        if (nb && g->overlap && since + room == ipe) {
            // these sweeps use up the ghost rows: their last pass hands the neighbours' rows over first and
            // the exchange runs beside the rest of it
            CCP_TRY(run_unchecked(g, room, nullptr, false, nullptr, g->desc.ghost));
            CCP_TRY(exchange(g, true));
        } else {
            CCP_TRY(run_unchecked(g, room));
        }
        left -= room;
    }
    return CCP_OK;
}

}  // namespace

int ccp_grid_attach_comm(ccp_grid *g, ccp_comm *c)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    mg_release(&g->mg);                              // the multigrid hierarchy belongs to the partition
    if (!c) {                                        // detach
        g->comm = nullptr;
        g->part.clear();
        g->up_rank = g->down_rank = -1;
        return CCP_OK;
    }
    if (c->device != g->device) return CCP_ERR_BAD_ARG;
    const RcclApi *api = rccl_api();
    if (!api) return CCP_ERR_RCCL;
    // every rank learns every block: the partition must be contiguous row blocks of one image, in rank order
    const int me[4] = {g->desc.row_begin, g->desc.row_count, g->desc.ghost,
                       g->desc.width ^ (g->desc.height << 1) ^ (g->desc.channels << 28) ^ ((g->desc.flags & CCP_GRID_DIRICHLET_MASK) << 27)};
    int *dev = reinterpret_cast<int *>(c->scratch.p);
    std::vector<int> all((size_t)4 * c->world);
    CCP_HIP(hipMemcpyAsync(dev + 4 * c->rank, me, sizeof(me), hipMemcpyHostToDevice, g->stream));
    CCP_RCCL(api->AllGather(dev + 4 * c->rank, dev, 4, ncclInt32, c->comm, g->stream));
    CCP_HIP(hipMemcpyAsync(all.data(), dev, sizeof(int) * all.size(), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    int next = 0;
    for (int r = 0; r < c->world; ++r) {
        if (all[4 * r] != next || all[4 * r + 2] != me[2] || all[4 * r + 3] != me[3]) return CCP_ERR_BAD_ARG;
        next += all[4 * r + 1];
    }
    if (next != g->desc.height) return CCP_ERR_BAD_ARG;
    g->up_rank = (c->rank > 0 && g->ghost_top > 0) ? c->rank - 1 : -1;
    g->down_rank = (c->rank + 1 < c->world && g->ghost_bottom > 0) ? c->rank + 1 : -1;
    if ((c->rank > 0) != (g->up_rank >= 0) || (c->rank + 1 < c->world) != (g->down_rank >= 0)) return CCP_ERR_STATE;   // a neighbour without ghost rows
    // what the neighbours' ghost zones take: their depth, clipped by the image border on their far side
    g->send_up = g->up_rank >= 0 ? std::min(g->desc.ghost, g->desc.height - g->desc.row_begin) : 0;
    g->send_down = g->down_rank >= 0 ? std::min(g->desc.ghost, g->desc.row_begin + g->desc.row_count) : 0;
    if (g->send_up > g->desc.row_count || g->send_down > g->desc.row_count) return CCP_ERR_UNSUPPORTED;   // block thinner than the ghost depth
    if (!g->stream_comm) {
        int lo = 0, hi = 0;                              // hi = greatest priority (numerically lowest)
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        CCP_HIP(hipStreamCreateWithPriority(&g->stream_comm, hipStreamNonBlocking, hi));
        CCP_HIP(hipEventCreateWithFlags(&g->ev_comm, hipEventDisableTiming));
        CCP_HIP(hipEventCreateWithFlags(&g->ev_ready, hipEventDisableTiming));
    }
    g->part.assign((size_t)c->world + 1, g->desc.height);
    for (int r = 0; r < c->world; ++r) g->part[(size_t)r] = all[4 * r];
    g->comm = c;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_overlap(ccp_grid *g, int32_t on)
try {
    CCP_TRY(not_weighted(g));
    if (!g) return CCP_ERR_BAD_ARG;
    g->overlap = on != 0;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_exchange_halos(ccp_grid *g)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    return exchange(g, false);
} CCP_ABI_CATCH

int ccp_grid_sweep_rowblocked(ccp_grid *g, int32_t iterations)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (iterations < 0) return CCP_ERR_BAD_ARG;
    if (!g->comm) return CCP_ERR_STATE;
    CCP_TRY(begin_timing(g));
    CCP_TRY(sweep_rowblocked(g, iterations));
    CCP_TRY(end_timing(g));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_residual_norm2_global(ccp_grid *g, double *rr_bb)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!rr_bb) return CCP_ERR_BAD_ARG;
    if (!g->comm) return CCP_ERR_STATE;
    const RcclApi *api = rccl_api();
    if (!api) return CCP_ERR_RCCL;
    if (has_neighbours(g) && g->half_sweeps_since_refresh > 0) CCP_TRY(exchange(g, false));   // A x needs current ghost rows
    CCP_TRY(residual_to_small(g));
    CCP_RCCL(api->AllReduce(g->small.p, g->small.p, (size_t)2 * g->desc.channels, ncclDouble, ncclSum, g->comm->comm, g->stream));
    return small_to_rr_bb(g, rr_bb);
} CCP_ABI_CATCH

int ccp_grid_gauss_seidel_rowblocked(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t check_every,
                                     ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!g->comm) return CCP_ERR_STATE;
    if (max_iteration < 0 || check_every < 0) return CCP_ERR_BAD_ARG;
    const RcclApi *api = rccl_api();
    if (!api) return CCP_ERR_RCCL;
    const int C = g->desc.channels;
    const bool nb = has_neighbours(g);
    const int ipe = std::max(1, g->desc.ghost / 2);
    double eps[kMaxChannels];
    int stop_at[kMaxChannels];
    for (int ch = 0; ch < C; ++ch) {
        eps[ch] = 10.0;                                   // `double eps = 10` (sparse-matrix.h:354)
        stop_at[ch] = 0;
    }
    CCP_TRY(begin_timing(g));
    int cnt = 0;
    auto any_above = [&]() {
        for (int ch = 0; ch < C; ++ch)
            if (stop_at[ch] == 0 && eps[ch] > epsilon) return true;
        return false;
    };
    if (check_every == 0) {
        if (10.0 > epsilon) {
            CCP_TRY(sweep_rowblocked(g, max_iteration));
            cnt = max_iteration;
        }
    } else if (g->fuse && !(getenv("CCP_GS_ROWBLOCK_CHECKED_FUSED") && atoi(getenv("CCP_GS_ROWBLOCK_CHECKED_FUSED")) == 0)) {
        // The rule after every check_every-th sweep at the speed of the temporally blocked pass: a checked pass reports the
        // step of each of its sweeps (as ccp_grid_gauss_seidel does on one block); the blocks' sums are all-reduced and
        // every rank takes the same decisions.  A channel freezes at the sweep its rule fired at (re-run from the pass's
        // input for the missing sweeps when that sweep lies inside a pass), exactly as on one block.
        SolveState host;
        CCP_TRY(start_solve_state(g, host));
        const size_t elems = (size_t)g->geom.ch_stride * C;
        CCP_TRY(ensure_checked_work(g));
        const bool shrinking = g->shrink_top || g->shrink_bottom;
        const int max_checked = g->masked ? kMaskedMaxCheckedT : kFusedMaxCheckedT;
        double *cur = g->x.p, *alt = g->x_alt.p;
        int was_active[kMaxChannels];
        for (int ch = 0; ch < C; ++ch) was_active[ch] = 1;
        bool any_active = (10.0 > epsilon) && max_iteration > 0;
        int k0 = 0;
        // every rank enters with fresh ghost rows: the depth of a pass follows from the ghost rows left, and the ranks must
        // agree on it (the all-reduce below carries T * C values)
        if (any_active && nb) CCP_TRY(exchange(g, false, cur));
        while (any_active && k0 < max_iteration) {
            // the ghost rows left decide how deep the pass may be; none left: refresh them in the buffer the iterate is in
            if (nb && shrinking && g->half_sweeps_since_refresh + 2 > g->desc.ghost) CCP_TRY(exchange(g, false, cur));
            int T = std::min(max_checked, max_iteration - k0);
            if (shrinking) T = std::min(T, (g->desc.ghost - g->half_sweeps_since_refresh) / 2);
            if (T < 1) return CCP_ERR_STATE;
            const int since0 = g->half_sweeps_since_refresh;
            CCP_TRY(checked_pass(g, T, cur, alt, k0, check_every, epsilon, [&](size_t count) -> int {
                CCP_RCCL(api->AllReduce(g->sweep_sums.p, g->sweep_sums.p, count, ncclDouble, ncclSum, g->comm->comm, g->stream));
                return CCP_OK;
            }));
            CCP_HIP(hipMemcpyAsync(&host, g->state.p, sizeof(host), hipMemcpyDeviceToHost, g->stream));
            CCP_HIP(hipStreamSynchronize(g->stream));
            CCP_TRY(settle_stopped(g, host, was_active, k0, T, cur, alt, since0, &any_active));
            k0 += T;
            std::swap(cur, alt);
        }
        if (cur != g->x.p) CCP_HIP(hipMemcpyAsync(g->x.p, cur, elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        cnt = k0;
        for (int ch = 0; ch < C; ++ch) {
            eps[ch] = host.last_eps[ch];
            stop_at[ch] = host.converged[ch] ? host.iterations[ch] : 0;
        }
    } else {
        // `while (eps > epsilon && cnt < max_iteration)` (sparse-matrix.h:356) with the step summed over all blocks
        while (any_above() && cnt < max_iteration) {
            const int plain = std::min(check_every - 1, max_iteration - cnt);
            if (plain > 0) {
                CCP_TRY(sweep_rowblocked(g, plain));
                cnt += plain;
            }
            if (cnt >= max_iteration) break;
            if (nb && g->half_sweeps_since_refresh / 2 >= ipe) CCP_TRY(exchange(g, false));
            long blocks[2] = {0, 0};
            CCP_TRY(one_iteration(g, true, nullptr, blocks));
            ++cnt;
            CCP_TRY(launch_check(g, blocks, 0.0, 0, nullptr, g->small.p));
            CCP_RCCL(api->AllReduce(g->small.p, g->small.p, (size_t)C, ncclDouble, ncclSum, g->comm->comm, g->stream));
            double host[kMaxChannels];
            CCP_HIP(hipMemcpyAsync(host, g->small.p, sizeof(double) * C, hipMemcpyDeviceToHost, g->stream));
            CCP_HIP(hipStreamSynchronize(g->stream));
            for (int ch = 0; ch < C; ++ch) {
                if (stop_at[ch]) continue;
                eps[ch] = host[ch];
                if (!(eps[ch] > epsilon)) stop_at[ch] = cnt;
            }
            if (getenv("CCP_GS_DEBUG")) fprintf(stderr, "[ccp_gs] rowblocked sweep %d: step %.17g (channel 0), epsilon %.17g\n", cnt, eps[0], epsilon);
        }
    }
    return finish_solve(g, report, [&](int ch, ccp_gs_report &r) {
        r.converged = stop_at[ch] ? 1 : 0;
        r.iterations = stop_at[ch] ? stop_at[ch] : cnt;
        r.last_l1_step = eps[ch];
    });
} CCP_ABI_CATCH

// conjugateGradient (sparse-matrix.h:396-434) on a row block: the three-vector loop of ccp_cg.hpp on the OWNED rows (one
// contiguous range of the planes), A applied to the owned rows with the direction's row above and below them fetched from
// the neighbours before every product (one image row per neighbour), every dot product all-reduced.
int ccp_grid_conjugate_gradient_rowblocked(ccp_grid *g, double epsilon, int32_t max_iteration, ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!g->comm) return CCP_ERR_STATE;
    if (max_iteration < 0) return CCP_ERR_BAD_ARG;
    const RcclApi *api = rccl_api();
    if (!api) return CCP_ERR_RCCL;
    const Geom &geo = g->geom;
    if ((g->up_rank >= 0 && g->ghost_top < 1) || (g->down_rank >= 0 && g->ghost_bottom < 1)) return CCP_ERR_STATE;
    const long n = geo.ch_stride;
    const size_t row = (size_t)2 * geo.pitch;
    const long off = (long)geo.own_lo * (long)row, n_own = (long)(geo.own_hi - geo.own_lo) * (long)row;
    CCP_TRY(ensure_cg_work(g));
    hipStream_t s = g->stream;
    dim3 grid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)(geo.own_hi - geo.own_lo), 2);
    // one row of `plane` to each neighbour's ghost row next to its owned rows, theirs into ours
    auto fetch_rows = [&](double *plane) -> int {
        if (g->up_rank < 0 && g->down_rank < 0) return CCP_OK;
        CCP_RCCL(api->GroupStart());
        ncclResult_t r = ncclSuccess;
        if (g->up_rank >= 0) {
            r = api->Send(plane + (size_t)geo.own_lo * row, row, ncclDouble, g->up_rank, g->comm->comm, s);
            if (r == ncclSuccess) r = api->Recv(plane + (size_t)(geo.own_lo - 1) * row, row, ncclDouble, g->up_rank, g->comm->comm, s);
        }
        if (g->down_rank >= 0 && r == ncclSuccess) {
            r = api->Send(plane + (size_t)(geo.own_hi - 1) * row, row, ncclDouble, g->down_rank, g->comm->comm, s);
            if (r == ncclSuccess) r = api->Recv(plane + (size_t)geo.own_hi * row, row, ncclDouble, g->down_rank, g->comm->comm, s);
        }
        const ncclResult_t e = api->GroupEnd();
        if (r != ncclSuccess) return rccl_fail(r, "ncclSend/ncclRecv", __FILE__, __LINE__);
        CCP_RCCL(e);
        g->exchanges++;
        return CCP_OK;
    };
    double *total = reinterpret_cast<double *>(g->comm->scratch.p);
    auto sums = [&](double *partial, int *count, const double **sum_at, int slot) -> int {
        hipLaunchKernelGGL(k_reduce_to_one, dim3(1), dim3(kBlock), 0, s, partial, (long)*count, total + slot);
        CCP_HIP(hipGetLastError());
        CCP_RCCL(api->AllReduce(total + slot, total + slot, 1, ncclDouble, ncclSum, g->comm->comm, s));
        *count = 1;
        *sum_at = total + slot;
        return CCP_OK;
    };
    for (int ch = 0; ch < g->desc.channels; ++ch) {
        CCP_HIP(hipMemsetAsync(g->cg_r.p, 0, sizeof(double) * n, s));
        CCP_HIP(hipMemsetAsync(g->cg_p.p, 0, sizeof(double) * n, s));
        CCP_HIP(hipMemsetAsync(g->cg_ap.p, 0, sizeof(double) * n, s));
        // the loop sees the owned range of every vector; the product goes back to the planes' bases
        auto spmv = [&](const double *in_own, double *out_own) -> int {
            double *in = const_cast<double *>(in_own) - off;
            double *out = out_own - off;
            CCP_TRY(fetch_rows(in));
            launch_apply<0>(g, grid, in, out, geo.own_lo);
            return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
        };
        auto spmv_dot = [&](const double *in_own, double *out_own, int *n_partials) -> int {
            *n_partials = 0;                             // (the loop runs its own dot pass over the owned range)
            return spmv(in_own, out_own);
        };
        if (cg_fused_mode() == 0) {
            CCP_TRY(cg_solve(spmv, spmv_dot, g->b.p + (long)ch * n + off, g->x.p + (long)ch * n + off, g->cg_r.p + off, g->cg_p.p + off,
                             g->cg_ap.p + off, n_own, epsilon, max_iteration, g->cg_state.p, g->partial.p, s, g->ev0, g->ev1,
                             report ? report + ch : nullptr, sums, true));
            continue;
        }
        // the fused loop (72 B per unknown and iteration, ccp_cg.hpp): pass A recomputes the direction of a row's
        // neighbours from r and the previous direction, so BOTH travel — one row of each per neighbour and iteration
        CCP_HIP(hipMemsetAsync(g->cg_p2.p, 0, sizeof(double) * n, s));
        const int march_rows = 32;
        const int own_rows = geo.own_hi - geo.own_lo;
        const dim3 mgrid((unsigned)((geo.pitch + 2L * kBlock - 1) / (2L * kBlock)), (unsigned)((own_rows + march_rows - 1) / march_rows));
        auto apply = [&](double *xv_own, const double *rv_own, const double *p_in_own, double *p_out_own, double *apv_own, int *n_partials) -> int {
            double *rv = const_cast<double *>(rv_own) - off, *p_in = const_cast<double *>(p_in_own) - off;
            CCP_TRY(fetch_rows(rv));
            CCP_TRY(fetch_rows(p_in));
            *n_partials = (int)(mgrid.x * mgrid.y);
            launch_apply_march(g, mgrid, xv_own - off, rv, p_in, p_out_own - off, apv_own - off, march_rows, geo.own_lo, geo.own_hi);
            return hipGetLastError() == hipSuccess ? CCP_OK : CCP_ERR_HIP;
        };
        CCP_TRY(cg_solve_fused(spmv, apply, g->b.p + (long)ch * n + off, g->x.p + (long)ch * n + off, g->cg_r.p + off, g->cg_p.p + off,
                               g->cg_p2.p + off, g->cg_ap.p + off, n_own, epsilon, max_iteration, g->cg_state.p, g->partial.p, s, g->ev0,
                               g->ev1, report ? report + ch : nullptr, sums, true));
    }
    // the ghost rows of x are stale now: the next sweep needs an exchange first
    g->half_sweeps_since_refresh = g->desc.ghost;
    return edge_timeout_status(g);
} CCP_ABI_CATCH

int ccp_grid_comm_stats(ccp_grid *g, int64_t *exchanges, int32_t *wait_mode, int32_t *send_up_rows, int32_t *send_down_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    if (exchanges) *exchanges = g->exchanges;
    if (wait_mode) *wait_mode = g->edge_flag ? g->wait_mode : -1;
    if (send_up_rows) *send_up_rows = g->send_up;
    if (send_down_rows) *send_down_rows = g->send_down;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_region_begin(ccp_grid *g)
try {
    CCP_TRY(bind(g));
    if (!g->ev_r0) {
        CCP_HIP(hipEventCreate(&g->ev_r0));
        CCP_HIP(hipEventCreate(&g->ev_r1));
    }
    g->region_launches = 0;
    g->region_iterations = 0;
    CCP_HIP(hipEventRecord(g->ev_r0, g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_region_end(ccp_grid *g, float *milliseconds, int64_t *sweep_launches, int64_t *pass_iterations)
try {
    CCP_TRY(bind(g));
    if (!g->ev_r0) return CCP_ERR_STATE;
    CCP_HIP(hipEventRecord(g->ev_r1, g->stream));
    CCP_HIP(hipEventSynchronize(g->ev_r1));
    float ms = 0.f;
    CCP_HIP(hipEventElapsedTime(&ms, g->ev_r0, g->ev_r1));
    if (milliseconds) *milliseconds = ms;
    if (sweep_launches) *sweep_launches = g->region_launches;
    if (pass_iterations) *pass_iterations = g->region_iterations;
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_last_timing(ccp_grid *g, float *milliseconds, int32_t *kernel_launches)
try {
    CCP_TRY(bind(g));
    if (g->timing_pending) {
        CCP_HIP(hipEventSynchronize(g->ev1));
        float ms = 0.f;
        CCP_HIP(hipEventElapsedTime(&ms, g->ev0, g->ev1));
        g->last_ms = ms;
        g->timing_pending = false;
    }
    if (milliseconds) *milliseconds = g->last_ms;
    if (kernel_launches) *kernel_launches = g->last_launches;
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"
