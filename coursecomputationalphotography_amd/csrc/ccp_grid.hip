// ccp_grid.hip — C ABI of the structured (matrix-free) Poisson grid path.  See include/ccp_gs.h.
#include "ccp_grid_kernels.hpp"
#include "ccp_grid_fused.hpp"
#include "ccp_grid_fused_wide.hpp"
#include "ccp_grid_lex.hpp"
#include "ccp_cg.hpp"
#include "ccp_grid_cg.hpp"
#include "ccp_grid_mg_view.hpp"
#include "ccp_grid_blend.hpp"
#include "ccp_grid_weighted_api.hpp"
#include "ccp_grid_adjoint.hpp"
#include "ccp_comm.hpp"
#include "ccp_view_check.hpp"
#include "ccp_grid_mask.hpp"

#include <algorithm>
#include <functional>
#include <cstring>
#include <chrono>
#include <vector>

using namespace ccp;

constexpr int kEdgeRing = 64;        // edge-counter slots (one per edge epoch, cleared together every kEdgeRing epochs)

struct ccp_grid {
    ccp_grid_desc desc{};
    Geom geom{};
    int ghost_top = 0, ghost_bottom = 0;
    // a side "shrinks" when the local block stops short of the image border there: its
    // outermost ghost row has no neighbour row, so validity recedes one row per half-sweep
    bool shrink_top = false, shrink_bottom = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;     // border tiles of a fused pass run here, beside the ordinary ones
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    // Row blocks with neighbours.  The pass that uses up the ghost rows finishes the owned rows the
    // neighbours need FIRST, inside the one launch (short edge chunks dispatched first): its waves count
    // themselves in *edge_counter and the last one publishes edge_epoch in *edge_flag (signal memory),
    // which the stream of the halo exchange waits for (ccp_grid_fused.hpp: fused_signal_edge).
    unsigned long long *edge_counter = nullptr;   // device memory: kEdgeRing counters, the pass of epoch e uses slot e % kEdgeRing
    unsigned long long *edge_flag = nullptr;      // hipMallocSignalMemory
    unsigned long long edge_epoch = 0;
    // Bounded device-side waits record giving up here (host-mapped memory): the polling kernel of wait_mode 1, which
    // gives up after edge_timeout_ticks (it must not hold a queue for ever when something — a profiler serialising
    // dispatches — keeps the pass from running beside it) and so lets the exchange send rows that may not be final;
    // and a wave of k_fused_multi whose input tiles never completed.  Every later call on the handle, and every call
    // that hands results to the host, then fails with CCP_ERR_STATE: a lost hand-off is an error, never a silently
    // wrong row.
    unsigned *edge_timeout = nullptr;
    unsigned long long edge_timeout_ticks = 200000000ull;   // 100 MHz constant clock: 2 s (CCP_GS_EDGE_TIMEOUT_TICKS)
    int wait_mode = 0;                   // 0: hipStreamWaitValue64, 1: a one-wave polling kernel (CCP_GS_EDGE_WAIT=spin, or no wait-value support)
    bool edge_signal = true;             // CCP_GS_EDGE_SIGNAL=0: the flag is only published after the whole pass
    // RCCL (ccp_grid_attach_comm): neighbour ranks, the rows their ghost zones take, the stream the
    // messages are issued on and the event the sweeps wait for
    ccp_comm *comm = nullptr;
    std::vector<int> part;               // every rank's first image row, then the image height (all-gathered at attach)
    int up_rank = -1, down_rank = -1;
    int send_up = 0, send_down = 0;
    hipStream_t stream_comm = nullptr;
    hipEvent_t ev_comm = nullptr, ev_ready = nullptr;
    bool overlap = true;                 // exchange beside the rest of the last pass (ccp_grid_set_overlap)
    long exchanges = 0;                  // halo exchanges issued (statistics)
    DevBuf<double> x, b;
    DevBuf<double> cg_r, cg_p, cg_p2, cg_ap;   // conjugate-gradient work vectors, one channel each (p double-buffered: fused loop)
    DevBuf<CgState> cg_state;
    DevBuf<double> x_alt;        // ping-pong partner of x for the temporally blocked sweep
    // The CSR entry point's grid twins (ccp_csr.hip) ask for their layout at every solve: for them a run of passes may
    // end in either buffer — x and x_alt then swap roles — instead of being planned as an EVEN number of launches
    // (50 iterations at depth 8: seven launches instead of eight).  Handles whose x_dev a caller may hold keep the parity.
    bool allow_swap = false;
    // Dirichlet-mask grid (CCP_GRID_DIRICHLET_MASK): uniform 5-point stencil on the pixels whose mask byte
    // is 1, everything else fixed at zero.  maskp: one byte per pixel in the layout of x (one channel);
    // tile_live: which tiles of the current tiling hold any unknown (k_masked_tile_census), cached per tiling.
    bool masked = false;
    DevBuf<unsigned char> maskp, tile_live;
    DevBuf<int> tile_rows;       // ... and which of a live tile's own rows do (two ints per tile)
    // the region bytes of image rows y0-1 and y0+local_rows (2 x W, zero where a row does not exist): the blend
    // assembly reads its neighbours there (ccp_grid_blend.hpp).  Known after ccp_grid_set_mask_host / _device, and
    // after the internal split-layout twin on a handle that holds the whole canvas.  mask_border: the region touches the
    // canvas's outer rows or columns (1 / 0; -1 not known yet -- the internal twin only -- computed at the first clone call).
    DevBuf<unsigned char> mask_edge;
    DevBuf<unsigned long long> mask_counters;   // ccp_grid_set_mask_device: owned unknowns, border flag
    bool mask_edge_known = false;
    int mask_border = -1;
    int live_T = -1, live_R = -1, live_lo = -1, live_hi = -1;
    long unknowns = 0;           // mask bytes set (owned rows), for the statistics
    bool fuse = true;            // use k_fused_sweep for unchecked sweeps
    int multi = 0;               // CCP_GS_MULTI=1: consecutive passes of equal depth as ONE launch (k_fused_multi)
    DevBuf<unsigned> multi_words; // its ticket and per-tile completion counters
    bool xcd_swizzle = false;    // CCP_GS_XCD=1: tiles of a pass in XCD-contiguous runs (measured 2-4 % slower at 16384^2: off)
    const char *trace_file = nullptr;   // CCP_GS_TRACE_FILE: per-wave start/end stamps of every fused pass are appended here (diagnostics; syncs)
    DevBuf<unsigned long long> trace;
    bool short_edges = true;     // chunk rows at an image edge are short (CCP_GS_SHORT_EDGES=0 turns it off)
    int side_rows_override = 0;  // CCP_GS_SIDE_ROWS
    int fuse_tmax = kFusedMaxT;  // iterations fused per launch (<= kFusedMaxT)
    int rows_per_chunk = 128;    // rows a fused wave finalises (plus 4T halo rows); default for every T
    // per-depth launch cost (ms) and chunk rows measured by ccp_grid_tune; index = T
    float tune_ms[kFusedMaxT + 1] = {0};
    int tune_rows[kFusedMaxT + 1] = {0};
    bool tuned = false;
    bool all_border = false;     // debug (CCP_GS_ALL_BORDER): every tile of a pass goes through k_fused_border
    bool force_border = false;   // debug (CCP_GS_FORCE_BORDER): and every trip there takes the border body
    bool red_store_all = false;  // A/B (CCP_GS_RED_STORE=1): every pass stores both colour halves (run_unchecked)
    bool wide = true;            // A/B (CCP_GS_WIDE=0): the depth-8 unchecked passes keep 128-px ordinary strips (k_fused_sweep)
    int cus = 0;                 // compute units of the device: k_fused_sweep_wide holds one wave per SIMD, 4 per CU
    int wide_segments = -1;      // A/B (CCP_GS_WIDE_SEGMENTS): -1 the planner (ccp_wide_plan.hpp), 0 the interior chunks, n > 0: n segments
    DevBuf<double> partial;      // per-block partial sums (L1 step / residual / checksums)
    long partial_region = 0;     // doubles per colour region of `partial` (L1 step)
    DevBuf<double> small;        // 4*kMaxChannels doubles of reduced results
    DevBuf<unsigned> io_bad;     // ccp_grid_assemble_from_images_device: set when a label selects no image
    DevBuf<double> sweep_sums;   // row blocks: step sums of every sweep of a checked pass (kFusedMaxCheckedT * kMaxChannels)
    DevBuf<SolveState> state;
    DevBuf<int> redo_mask;       // per-channel flags for re-running one channel of a checked pass
    // lexicographic (reference-order) path: diagonal-major copies of x and b, snapshot, step sums
    DevBuf<double> lex_x, lex_b, lex_snap, lex_partial, lex_eps;
    DevBuf<unsigned> lex_progress, lex_ticket;   // strip-wave pipeline: diagonals finished per (channel, sweep, strip); work tickets
    DevBuf<double> lex_edges;    // time-skewed strips: results of each strip's lanes 62/63 per step and sweep (read by the strip to its right)
    int lex_mode = 3;            // 3: time-skewed strips, the T sweeps of a pass on the T waves of a workgroup (k_lex_wg, default);
                                 // CCP_GS_LEX_MODE=planes -> 0: one launch per hyperplane (k_lex_plane, the independent engine)
    int lex_tmax = 8;            // deepest time-skewed pass
                                 // k_lex_wg: ticket -> group * strips + strip, in the order the strips can start:
    unsigned *lex_order_pin = nullptr;   // ... built here, in pinned host memory the kernel reads directly (one word per strip, long before
    unsigned *lex_order_dev = nullptr;   //     the strip's gate opens): copying 34 KB to the device cost 7-8 ms of host time inside the timing
    size_t lex_order_pin_cap = 0;        //     of a 256-sweep solve, from pageable and from pinned memory alike (CCP_GS_DEBUG laps, round 4)
    size_t lex_order_count = 0;
    int lex_order_groups = 0, lex_order_strips = 0, lex_order_depth = 0;
    LexGeom lexg{};
    DevBuf<double> stage;        // natural-order staging rows for host transfers
    long stage_rows = 0;
    int half_sweeps_since_refresh = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_r0 = nullptr, ev_r1 = nullptr;   // ccp_grid_region_begin / _end (created on first use)
    long region_launches = 0;    // passes / half-sweep launches since ccp_grid_region_begin
    long region_iterations = 0;  // iterations those passes performed (sum of their depths)
    float last_ms = 0.f;
    int last_launches = 0;
    bool timing_pending = false;
    int cpt = 2;                 // half-columns per thread of the sweep kernel
    int rows_per_block = 32;
    MgHierarchy *mg = nullptr;   // multigrid hierarchy (ccp_grid_mg.hip), built at the first ccp_grid_mg_* call
    // Weighted grid (CCP_GRID_WEIGHTED, ccp_grid_weighted.hpp): the level-0 operator in four planes of one channel's layout
    // (d, we, ws, lambda), valid once ccp_grid_set_weights_* has accepted one (has_op); wpart: the residual's partial sums
    bool weighted = false;
    bool has_op = false;
    DevBuf<double> wop, wpart;
    // Fixed pixels (ccp_grid_set_weights_constrained_*): wcons holds the planes ce, cs and lambda' (ccp_grid_weighted.hpp)
    // while the operator has any (has_fixed), and is released otherwise.  wcount: the formation pass's verdict and counts
    bool has_fixed = false;
    DevBuf<double> wcons;
    DevBuf<unsigned long long> wcount;
    // One operator per channel (ccp_grid_set_weights_per_channel_device): wop then holds `channels` sets of the four planes,
    // 4 x ch_stride apart, and wcons (while any channel has a fixed pixel) `channels` sets of its three, 3 x ch_stride
    // apart.  op_sets: the sets wop holds now, 1 after the shared operator's setters.  pc_*: ccp_grid_constraint_info's
    // figures of every set, index 0 the shared operator's (pc_live < 0: not counted yet).
    bool per_channel = false;
    int op_sets = 1;
    long pc_fixed[kMaxChannels] = {}, pc_live[kMaxChannels] = {}, pc_edges[kMaxChannels] = {};
    MgConfig mg_cfg;                           // ccp_grid_mg_set_* (ccp_grid_mg_view.hpp)
    MgNullspace mg_nullspace;                  // goes with the operator (drop_operator)
};

namespace {

constexpr int kWeightedApplyBlocks = 1024;   // blocks per (channel, colour) of k_weighted_apply

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

int zero_unmasked(ccp_grid *g, double *plane)
{
    if (!g->masked) return CCP_OK;
    hipLaunchKernelGGL(k_zero_unmasked, dim3(2048, 1, (unsigned)g->desc.channels), dim3(kBlock), 0, g->stream, plane, g->maskp.p,
                       g->geom.ch_stride);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// What every mask setter does once the new mask bytes are enqueued: what was derived from the old mask goes, and x, b
// and x_alt are zeroed outside the new region.
int mask_replaced(ccp_grid *g)
{
    g->live_T = -1;                                      // the tile census belongs to the old mask
    mg_release(&g->mg);                                  // ... and so does the multigrid hierarchy
    CCP_TRY(zero_unmasked(g, g->x.p));
    CCP_TRY(zero_unmasked(g, g->b.p));
    if (g->x_alt.p) CCP_TRY(zero_unmasked(g, g->x_alt.p));
    return CCP_OK;
}

// k_weighted_apply: up to kWeightedApplyBlocks blocks per (channel, colour) striding over the colour's cells
dim3 weighted_apply_grid(const ccp_grid *g)
{
    const long cells = (long)g->geom.H * ((g->geom.W + 1) / 2);
    return dim3((unsigned)std::max<long>(1, std::min<long>(kWeightedApplyBlocks, (cells + kBlock - 1) / kBlock)), 1, 2 * (unsigned)g->desc.channels);
}

// b := A x (MODE 0) or the residual's partial sums (MODE 1) of every channel of a weighted handle.  With one operator
// per channel the same kernel runs once per channel on that channel's planes, vectors and slice of the partial sums:
// the launch a one-channel handle makes.
template <int MODE>
int weighted_apply(ccp_grid *g)
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

// ---- Steps the solve entry points share (NOTES.md §R22.1).  The drivers around them stay apart: the one-block loop runs one
// ---- pass ahead of the host, the row-block loop is synchronous, row-block CG fetches ghost rows and all-reduces.

// The end of every solve: the end event, the wait, the time, then the reports.  per_channel(ch, r) fills report[ch]'s
// converged / iterations / last_l1_step from wherever the caller keeps them.  state_out: the device's SolveState is read
// back into it between the end event and the wait (the one-block solve's last look at it).
template <class PerChannel>
int finish_solve(ccp_grid *g, ccp_gs_report *report, PerChannel per_channel, SolveState *state_out = nullptr)
{
    CCP_TRY(end_timing(g));
    if (state_out) CCP_HIP(hipMemcpyAsync(state_out, g->state.p, sizeof(*state_out), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    float ms = 0.f;
    CCP_HIP(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    g->last_ms = ms;
    g->timing_pending = false;
    for (int ch = 0; report && ch < g->desc.channels; ++ch) {
        per_channel(ch, report[ch]);
        report[ch].seconds = ms * 1e-3;
    }
    return CCP_OK;
}

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

// Host <-> device rows in natural order through the staging buffer.
template <bool TO_DEVICE>
int transfer_rows(ccp_grid *g, double *dev_base, int channel, double *rows, int first_row, int n_rows)
{
    CCP_TRY(bind(g));
    if (!rows || channel < 0 || channel >= g->desc.channels || n_rows < 0) return CCP_ERR_BAD_ARG;
    const int img_lo = g->geom.y0, img_hi = g->geom.y0 + g->geom.local_rows;
    if (first_row < img_lo || first_row + n_rows > img_hi) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width;
    int done = 0;
    while (done < n_rows) {
        const int chunk = (int)std::min<long>(g->stage_rows, n_rows - done);
        const int l_first = first_row + done - g->geom.y0;
        dim3 grid((unsigned)((W + kBlock - 1) / kBlock), (unsigned)chunk);
        const size_t bytes = (size_t)chunk * W * sizeof(double);
        double *host = rows + (size_t)done * W;
        if (TO_DEVICE) {
            CCP_HIP(hipMemcpyAsync(g->stage.p, host, bytes, hipMemcpyHostToDevice, g->stream));
            hipLaunchKernelGGL((k_convert<true>), grid, dim3(kBlock), 0, g->stream, dev_base, g->stage.p,
                               g->geom, channel, l_first, W);
            CCP_HIP(hipGetLastError());
        } else {
            hipLaunchKernelGGL((k_convert<false>), grid, dim3(kBlock), 0, g->stream, dev_base, g->stage.p,
                               g->geom, channel, l_first, W);
            CCP_HIP(hipGetLastError());
            CCP_HIP(hipMemcpyAsync(host, g->stage.p, bytes, hipMemcpyDeviceToHost, g->stream));
        }
        CCP_HIP(hipStreamSynchronize(g->stream));
        done += chunk;
    }
    return edge_timeout_status(g);
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

int ccp_grid_set_b_host(ccp_grid *g, int32_t channel, const double *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    CCP_TRY(transfer_rows<true>(g, g->b.p, channel, const_cast<double *>(rows), first_row, n_rows));
    return zero_unmasked(g, g->b.p);
} CCP_ABI_CATCH

int ccp_grid_set_x_host(ccp_grid *g, int32_t channel, const double *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    CCP_TRY(transfer_rows<true>(g, g->x.p, channel, const_cast<double *>(rows), first_row, n_rows));
    return zero_unmasked(g, g->x.p);
} CCP_ABI_CATCH

int ccp_grid_get_x_host(ccp_grid *g, int32_t channel, double *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return transfer_rows<false>(g, g->x.p, channel, rows, first_row, n_rows);
} CCP_ABI_CATCH

int ccp_grid_get_b_host(ccp_grid *g, int32_t channel, double *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return transfer_rows<false>(g, g->b.p, channel, rows, first_row, n_rows);
} CCP_ABI_CATCH

int ccp_grid_set_mask_host(ccp_grid *g, const uint8_t *mask, int64_t row_stride_bytes)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!g->masked) return CCP_ERR_STATE;
    if (!mask || row_stride_bytes < g->desc.width) return CCP_ERR_BAD_ARG;
    const Geom &geo = g->geom;
    std::vector<unsigned char> split((size_t)geo.ch_stride, 0);
    long count = 0;
    for (int l = 0; l < geo.local_rows; ++l) {
        const int y = geo.y0 + l;
        const uint8_t *row = mask + (size_t)y * (size_t)row_stride_bytes;
        for (int x = 0; x < geo.W; ++x) {
            if (!row[x]) continue;
            split[(size_t)(((long)l * 2 + ((x + y) & 1)) * geo.pitch + (x >> 1))] = 1;
            if (l >= geo.own_lo && l < geo.own_hi) ++count;
        }
    }
    // the rows just beyond the local ones, and whether the region reaches the canvas's outer rows or columns
    // (every block is handed the whole mask, so every block finds the same answer)
    std::vector<unsigned char> edge(2 * (size_t)geo.W, 0);
    const int y_above = geo.y0 - 1, y_below = geo.y0 + geo.local_rows;
    for (int x = 0; x < geo.W; ++x) {
        if (y_above >= 0) edge[x] = mask[(size_t)y_above * (size_t)row_stride_bytes + x] != 0;
        if (y_below < geo.H) edge[geo.W + x] = mask[(size_t)y_below * (size_t)row_stride_bytes + x] != 0;
    }
    bool border = false;
    for (int y = 0; y < geo.H && !border; ++y) {
        const uint8_t *row = mask + (size_t)y * (size_t)row_stride_bytes;
        if (row[0] || row[geo.W - 1]) border = true;
        if (y == 0 || y == geo.H - 1)
            for (int x = 0; x < geo.W && !border; ++x) border = row[x] != 0;
    }
    CCP_HIP(hipMemcpyAsync(g->maskp.p, split.data(), split.size(), hipMemcpyHostToDevice, g->stream));
    CCP_HIP(hipMemcpyAsync(g->mask_edge.p, edge.data(), edge.size(), hipMemcpyHostToDevice, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    g->mask_edge_known = true;
    g->mask_border = border ? 1 : 0;
    g->unknowns = count;
    CCP_TRY(mask_replaced(g));
    return CCP_OK;
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

// Library-internal twin of ccp_grid_set_mask_host for a mask that is already on the device in the grid's layout
// (the region recognition builds it there: ccp_csr.hip).  Asynchronous on the handle's stream.
int ccp::grid_set_allow_swap(ccp_grid *g, bool on)
{
    if (!g) return CCP_ERR_BAD_ARG;
    g->allow_swap = on;
    return CCP_OK;
}

int ccp::grid_set_mask_split_device(ccp_grid *g, const unsigned char *split_mask_dev, long unknowns)
{
    CCP_TRY(bind(g));
    if (!g->masked) return CCP_ERR_STATE;
    if (!split_mask_dev) return CCP_ERR_BAD_ARG;
    CCP_HIP(hipMemcpyAsync(g->maskp.p, split_mask_dev, (size_t)g->geom.ch_stride, hipMemcpyDeviceToDevice, g->stream));
    // no rows beyond the local ones on a whole-canvas handle; a row block cannot tell (the blend calls refuse it)
    CCP_HIP(hipMemsetAsync(g->mask_edge.p, 0, 2 * (size_t)g->geom.W, g->stream));
    g->mask_edge_known = g->geom.y0 == 0 && g->geom.local_rows == g->geom.H;
    g->mask_border = -1;
    g->unknowns = unknowns;
    CCP_TRY(mask_replaced(g));
    CCP_HIP(hipStreamSynchronize(g->stream));            // the caller's buffer may go
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
        return weighted_apply<0>(g);
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

namespace {

// `iterations` lexicographic sweeps of the channels in `mask`, pipelined over the hyperplanes
// tau = x + y + 2k (ccp_grid_lex.hpp).  partial != nullptr: per-sweep step sums are written too.
// partial sums one checked sweep writes per channel
// (time-skewed strips: the strip count depends on the depth; the partial layout uses the largest, depth 8's —
// slots a shallower launch does not write must read as zero, so the buffer is cleared per batch)
// Tickets of a launch of `groups` groups of T sweeps on an image W pixels wide, in the order the strips can start: (k, s)
// follows its left neighbour (k, s-1) by a strip lag (the 62 diagonals its first pixel lies further on + the 16 steps of
// edge values it wants to see published + the publication's own lag) and the same strip of the group before by a group
// lag; a workgroup that is resident but waiting keeps a slot from one that could run.  Everything a strip waits for —
// (k, s-1), (k-1, s), the last reader of its edge buffer (k - kLexEdgeSets, s+1): lex_wg_body — holds a smaller ticket, and a
// ticket's holder never waits for a larger one: no deadlock, whatever the residency (tests/test_lex_tickets.py checks
// exactly that through ccp_debug_lex_tickets).  order[ticket] = k * strips + s, strips = lex_strip_count(W, T, groups).
void lex_ticket_order(int W, int T, int groups, std::vector<unsigned> &order)
{
    const int S = lex_strip_count(W, T, groups);
    const long strip_lag = kLexSkewCols + 34, group_lag = 19 + 4 * (T - 1) + 16;
    struct Ticket { long start; int k, s; };
    std::vector<long> start((size_t)groups * S, -1);
    std::vector<Ticket> tickets;
    for (int k = 0; k < groups; ++k)
        for (int st = lex_strip_first(T, k); st <= lex_strip_last(W, T, k); ++st) {
            long t = 0;
            if (lex_strip_exists(W, T, k, st - 1)) t = std::max(t, start[(size_t)k * S + st - 1] + strip_lag);
            if (lex_strip_exists(W, T, k - 1, st)) t = std::max(t, start[(size_t)(k - 1) * S + st] + group_lag);
            if (lex_strip_exists(W, T, k - kLexEdgeSets, st + 1)) t = std::max(t, start[(size_t)(k - kLexEdgeSets) * S + st + 1] + 1);
            start[(size_t)k * S + st] = t;
            tickets.push_back({t, k, st});
        }
    std::stable_sort(tickets.begin(), tickets.end(), [](const Ticket &a, const Ticket &b) { return a.start < b.start; });
    order.clear();
    for (const Ticket &t : tickets) order.push_back((unsigned)((long)t.k * S + t.s));
}

// the diagonal-major arrays behind their front rows (kLexFrontRows: what k_lex_wg's loader prefetches for a strip that
// starts left of the image lies up to 64 diagonals before the first one; never used)
double *lex_xd(const ccp_grid *g) { return g->lex_x.p + (size_t)kLexFrontRows * g->lexg.P; }
double *lex_bd(const ccp_grid *g) { return g->lex_b.p + (size_t)kLexFrontRows * g->lexg.P; }
constexpr int kLexBatchSweeps = 128;     // sweeps in flight between two looks at the stop rule: the first batch (later ones grow while the rule is far off)
constexpr int kLexLaunchSweeps = 1024;   // most sweeps one launch of k_lex_wg carries (its strips move 2 columns left per sweep: lex_strip_count)
long lex_partials_per_sweep(const ccp_grid *g)
{
    if (g->lex_mode == 3) return (long)lex_strip_count(g->desc.width, 1, kLexLaunchSweeps);   // (the groups of a checked batch shift by 2 x its sweeps at most)
    return (long)g->lexg.n_diag * g->lexg.nbx;
}

// `iterations` lexicographic sweeps as time-skewed strips: groups of T sweeps per pass through memory (k_lex_wg),
// T = 8, 4, 2, 1 for what is left over; every depth is one launch holding all its groups.
extern "C++" {
template <int T>
int lex_launch_skew(ccp_grid *g, int groups, unsigned mask, double *partial, int t_last = T)
{
    const LexGeom &lg = g->lexg;
    const int C = g->desc.channels;
    if ((long)groups * T > kLexLaunchSweeps) return CCP_ERR_STATE;
    const bool dbg = getenv("CCP_GS_DEBUG") != nullptr;
    const auto t_in = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (dbg) fprintf(stderr, "[ccp_gs] lex_launch_skew %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count());
    };
    const int S = lex_strip_count(lg.W, T, groups);                      // strip slots per group (not every group has all of them)
    const int S_cap = lex_strip_count(lg.W, 1, kLexLaunchSweeps);       // ... of the largest launch, whatever its depth
    const long edge_steps = kWave + lg.H + 2 * (T - 1);
    // persistent workgroups: as many as are resident at once (k_lex_wg's comment), each taking strips from the ticket counter
    int per_cu = 0, cus = 0;
    if (g->masked) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_lex_wg_masked<T, false>, (T + 2) * kWave, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_lex_wg<T, false>, (T + 2) * kWave, 0);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device);
    const long resident = (long)std::max(per_cu, 1) * std::max(cus, 1);
    lap("occupancy known");
    // Buffers are sized for the largest launch a solve can issue (kLexLaunchSweeps), not for this one: a call with more
    // sweeps than the call before must not pay a 0.5 GB reallocation inside its own timing (the kernel trace of round 4
    // showed 25 ms of it between the layout conversion and the launch).
    const size_t need = (size_t)C * groups * S * kLexWordStride;
    const size_t need_cap = (size_t)C * std::max(groups, kLexLaunchSweeps / 8) * S_cap * kLexWordStride;
    const size_t edges = (size_t)kLexEdgeSets * C * S * edge_steps * 2 * T + (size_t)C * resident * kLexScratch;   // (+ the storers' scratch slots, one set per resident workgroup)
    const size_t edges_cap = (size_t)kLexEdgeSets * C * S_cap * (kWave + lg.H + 14) * 16 + (size_t)C * resident * kLexScratch;   // (what depth 8 needs)
    if (g->lex_progress.n < need) CCP_TRY(g->lex_progress.alloc(std::max(need, need_cap)));
    if (g->lex_order_groups != groups || g->lex_order_strips != S || g->lex_order_depth != T) {
        // Tickets in the order the strips can start: (k, s) follows its left neighbour (k, s-1) by a strip lag (the 62
        // diagonals its first pixel lies further on + the 16 steps of edge values it wants to see published + the
        // publication's own lag) and the same strip of the group before by a group lag; a workgroup that is resident but
        // waiting keeps a slot from one that could run.  Everything a strip waits for holds a smaller ticket — a ticket's
        // holder never waits for a larger one: no deadlock, whatever the residency.
        std::vector<unsigned> tickets;
        lex_ticket_order(lg.W, T, groups, tickets);
        if (tickets.empty()) return CCP_ERR_STATE;
        lap("tickets sorted");
        const size_t order_cap = std::max(tickets.size(), (size_t)(kLexLaunchSweeps / 8) * S_cap);
        CCP_HIP(hipStreamSynchronize(g->stream));               // (an earlier copy from the pinned buffer may still be in flight)
        lap("stream drained");
        if (g->lex_order_pin_cap < tickets.size()) {
            if (g->lex_order_pin) (void)hipHostFree(g->lex_order_pin);
            g->lex_order_pin = g->lex_order_dev = nullptr;
            g->lex_order_pin_cap = 0;
            CCP_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->lex_order_pin), order_cap * sizeof(unsigned), hipHostMallocMapped));
            CCP_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&g->lex_order_dev), g->lex_order_pin, 0));
            g->lex_order_pin_cap = order_cap;
        }
        for (size_t i = 0; i < tickets.size(); ++i) g->lex_order_pin[i] = tickets[i];
        __atomic_thread_fence(__ATOMIC_RELEASE);
        g->lex_order_count = tickets.size();
        g->lex_order_groups = groups;
        g->lex_order_strips = S;
        g->lex_order_depth = T;
        lap("order queued");
    }
    const unsigned n_tickets = (unsigned)g->lex_order_count;
    const long wgs = std::max<long>(1, std::min<long>((long)n_tickets, (resident + C - 1) / C));
    if (g->lex_edges.n < edges) CCP_TRY(g->lex_edges.alloc(std::max(edges, edges_cap)));
    if (!g->lex_ticket.p) CCP_TRY(g->lex_ticket.alloc(kMaxChannels));
    CCP_HIP(hipMemsetAsync(g->lex_progress.p, 0, need * sizeof(unsigned), g->stream));
    CCP_HIP(hipMemsetAsync(g->lex_ticket.p, 0, kMaxChannels * sizeof(unsigned), g->stream));
    dim3 grid((unsigned)wgs, (unsigned)C);
    lap("buffers cleared");
    if (getenv("CCP_GS_DEBUG"))
        fprintf(stderr, "[ccp_gs] k_lex_wg<%d>: %d workgroups per CU on %d CUs, %ld persistent workgroups per channel for %d groups x %d strips\n",
                T, per_cu, cus, wgs, groups, S);
    const dim3 block((T + 2) * kWave);
    double *nop = nullptr;
    unsigned long long *trace = nullptr;
    const size_t trace_words = (size_t)4 * C * groups * S;
    if (g->trace_file) {
        if (g->trace.n < trace_words) CCP_TRY(g->trace.alloc(trace_words));
        CCP_HIP(hipMemsetAsync(g->trace.p, 0, trace_words * sizeof(unsigned long long), g->stream));
        trace = g->trace.p;
    }
#define CCP_LEX_WG(KERNEL, CHECK, P, STRIDE)                                                                                        \
    hipLaunchKernelGGL((KERNEL<T, CHECK>), grid, block, 0, g->stream,                                                                \
                       LexWgArgs{lex_xd(g), lex_bd(g), g->geom, lg, groups, S, n_tickets, g->lex_progress.p, g->lex_ticket.p, g->lex_order_dev,  \
                                 g->lex_edges.p, edge_steps, mask, P, STRIDE, trace, t_last})
    if (g->masked) {
        if (partial) CCP_LEX_WG(k_lex_wg_masked, true, partial, lex_partials_per_sweep(g));
        else CCP_LEX_WG(k_lex_wg_masked, false, nop, 0L);
    } else {
        if (partial) CCP_LEX_WG(k_lex_wg, true, partial, lex_partials_per_sweep(g));
        else CCP_LEX_WG(k_lex_wg, false, nop, 0L);
    }
#undef CCP_LEX_WG
    CCP_HIP(hipGetLastError());
    if (trace) {
        CCP_HIP(hipStreamSynchronize(g->stream));
        std::vector<unsigned long long> host(trace_words);
        CCP_HIP(hipMemcpy(host.data(), trace, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(g->trace_file, "ab")) {
            // (the same 8-word header as the fused passes' records, tag "LEXTRAC")
            const unsigned long long head[8] = {0x4341525458454cull, (unsigned long long)T, (unsigned long long)groups, (unsigned long long)S,
                                                (unsigned long long)C, (unsigned long long)lg.H, (unsigned long long)host.size(), (unsigned long long)lg.W};
            fwrite(head, sizeof(head), 1, f);
            fwrite(host.data(), sizeof(unsigned long long), host.size(), f);
            fclose(f);
        }
    }
    return CCP_OK;
}
}  // extern "C++"

int lex_run_skew(ccp_grid *g, int iterations, unsigned mask, double *partial)
{
    const int C = g->desc.channels;
    const long per_sweep = (long)C * lex_partials_per_sweep(g);          // partial doubles per sweep (all channels)
    int left = iterations, done = 0;
    if (g->lex_tmax >= 8 && left >= 8 && left % 8 != 0) {
        // a count that is not a multiple of 8: ONE launch of depth-8 groups whose last group passes the sweeps it does
        // not have through (lex_wg_pass_through) instead of remainder launches of depth 4, 2, 1, each a pipeline of its
        // own to fill and drain.  (With the stop rule too: the passed-through sweeps leave step sums of 0 in slots
        // beyond the batch's last sweep, which nobody reads; the partial buffer holds whole groups.)
        const int groups = (left + 7) / 8;
        return lex_launch_skew<8>(g, groups, mask, partial, left - 8 * (groups - 1));
    }
    for (int T = 8; T >= 1; T >>= 1) {
        if (T > g->lex_tmax || left < T) continue;
        const int groups = left / T;
        double *p = partial ? partial + (long)done * per_sweep : nullptr;
        if (T == 8) CCP_TRY(lex_launch_skew<8>(g, groups, mask, p));
        else if (T == 4) CCP_TRY(lex_launch_skew<4>(g, groups, mask, p));
        else if (T == 2) CCP_TRY(lex_launch_skew<2>(g, groups, mask, p));
        else CCP_TRY(lex_launch_skew<1>(g, groups, mask, p));
        done += groups * T;
        left -= groups * T;
    }
    return CCP_OK;
}

int lex_run(ccp_grid *g, int iterations, unsigned mask, double *partial)
{
    if (g->lex_mode == 3 && iterations > 0) return lex_run_skew(g, iterations, mask, partial);
    const LexGeom &lg = g->lexg;
    const int d_max = lg.n_diag - 1;
    const int C = g->desc.channels;
    for (int tau = 0; tau <= d_max + 2 * (iterations - 1); ++tau) {
        const int k_lo = std::max(0, (tau - d_max + 1) / 2);          // smallest k with tau - 2k <= d_max
        const int k_hi = std::min(iterations - 1, tau / 2);           // largest k with tau - 2k >= 0
        if (k_hi < k_lo) continue;
        dim3 grid((unsigned)lg.nbx, (unsigned)(k_hi - k_lo + 1), (unsigned)C);
        if (partial)
            hipLaunchKernelGGL((k_lex_plane<true>), grid, dim3(kBlock), 0, g->stream, lex_xd(g), lex_bd(g), g->geom, lg,
                               tau, k_lo, mask, partial);
        else
            hipLaunchKernelGGL((k_lex_plane<false>), grid, dim3(kBlock), 0, g->stream, lex_xd(g), lex_bd(g), g->geom, lg,
                               tau, k_lo, mask, static_cast<double *>(nullptr));
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

}  // namespace

int ccp_grid_gauss_seidel_lexicographic(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t check_every,
                                        ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (g->ghost_top || g->ghost_bottom || g->desc.row_count != g->desc.height) return CCP_ERR_STATE;   // whole image only
    if (g->masked && g->lex_mode != 3) return CCP_ERR_UNSUPPORTED;  // Dirichlet masks: k_lex_wg only
    if (max_iteration < 0 || check_every < 0) return CCP_ERR_BAD_ARG;
    const int C = g->desc.channels, W = g->desc.width, H = g->desc.height;
    LexGeom &lg = g->lexg;
    lg.W = W;
    lg.H = H;
    lg.P = ((long)W + 15) / 16 * 16;
    lg.n_diag = W + H - 1;
    lg.plane = (long)lg.n_diag * lg.P;
    lg.nbx = (std::min(W, H) + kLexTile - 1) / kLexTile;
    const size_t elems = (size_t)lg.plane * C;
    const size_t slack = (size_t)kLexSlackRows * lg.P;       // k_lex_wg prefetches some diagonals past the last one (never used)
    const size_t front = (size_t)kLexFrontRows * lg.P;       // ... and a strip that starts left of the image some diagonals before the first
    if (g->lex_x.n != front + elems + slack) {
        CCP_TRY(g->lex_x.alloc(front + elems + slack));
        CCP_TRY(g->lex_b.alloc(front + elems + slack));
        CCP_HIP(hipMemsetAsync(g->lex_x.p, 0, front * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(g->lex_b.p, 0, front * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(lex_xd(g) + elems, 0, slack * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(lex_bd(g) + elems, 0, slack * sizeof(double), g->stream));
    }
    CCP_TRY(begin_timing(g));
    dim3 cgrid((unsigned)((W + kBlock - 1) / kBlock), (unsigned)H, (unsigned)C);
    dim3 tgrid((unsigned)((W + kLexCT - 1) / kLexCT), (unsigned)((H + kLexCT - 1) / kLexCT), (unsigned)C);
    dim3 sgrid((unsigned)((W + kLexCT - 1) / kLexCT), (unsigned)((lg.n_diag + kLexCT - 1) / kLexCT), (unsigned)C);
    hipLaunchKernelGGL(k_lex_to_diag_sheared, sgrid, dim3(kBlock), 0, g->stream, g->x.p, lex_xd(g), g->geom, lg);
    if (g->masked) hipLaunchKernelGGL(k_lex_convert_b_masked, cgrid, dim3(kBlock), 0, g->stream, g->b.p, g->maskp.p, lex_bd(g), g->geom, lg);
    else hipLaunchKernelGGL(k_lex_to_diag_sheared, sgrid, dim3(kBlock), 0, g->stream, g->b.p, lex_bd(g), g->geom, lg);
    CCP_HIP(hipGetLastError());

    const unsigned all = (C >= 32) ? 0xffffffffu : ((1u << C) - 1u);
    int iterations_of[kMaxChannels], converged[kMaxChannels];
    double last_eps[kMaxChannels];
    for (int ch = 0; ch < C; ++ch) {
        iterations_of[ch] = max_iteration;
        converged[ch] = 0;
        last_eps[ch] = 10.0;                                              // `double eps = 10` (sparse-matrix.h:354)
    }
    if (check_every == 0 || !(10.0 > epsilon)) {
        // fixed count — or the reference loop never starts (eps = 10 <= epsilon)
        const int n = check_every == 0 ? max_iteration : 0;
        for (int done = 0; done < n;) {                    // gridDim.y carries the sweeps in flight: keep it small
            const int kb = std::min(g->lex_mode != 0 ? kLexLaunchSweeps : 32768, n - done);   // (k_lex_wg: one progress word per group and strip)
            CCP_TRY(lex_run(g, kb, all, nullptr));
            done += kb;
        }
        for (int ch = 0; ch < C; ++ch) iterations_of[ch] = n;
    } else {
        // Sweeps in flight between two looks at the rule: kLexBatchSweeps to begin with, doubled (up to one launch's worth)
        // while every channel's step, at the rate it has been shrinking, is more than four batches away from epsilon.  A
        // batch is one pipeline to fill and drain and one snapshot; a channel that stops inside a batch is redone from the
        // snapshot for exactly the sweeps the reference would have made — the result does not depend on the batching.  (The
        // reference's defaults, epsilon 1e-6 and 1,000 sweeps, never stop early on an image-sized system: 8 batches of 128
        // were 7.0 ms at 512^2 where one pipeline of 1,000 sweeps is 2.5 ms.)
        const int batch_cap = g->lex_mode == 3 ? kLexLaunchSweeps : kLexBatchSweeps;
        int batch = kLexBatchSweeps;
        const long per = lex_partials_per_sweep(g);                         // partials per (iteration, channel)
        if (g->lex_partial.n != (size_t)per * batch_cap * C) CCP_TRY(g->lex_partial.alloc((size_t)per * batch_cap * C));
        if (g->lex_eps.n != (size_t)batch_cap * C) CCP_TRY(g->lex_eps.alloc((size_t)batch_cap * C));
        if (g->lex_snap.n != elems) CCP_TRY(g->lex_snap.alloc(elems));
        std::vector<double> eps_vec((size_t)batch_cap * C);
        double *eps_host = eps_vec.data();
        unsigned mask = all;
        int done = 0;
        while (mask && done < max_iteration) {
            const int kb = std::min(batch, max_iteration - done);
            CCP_HIP(hipMemcpyAsync(g->lex_snap.p, lex_xd(g), elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
            if (g->lex_mode == 3) CCP_HIP(hipMemsetAsync(g->lex_partial.p, 0, sizeof(double) * (size_t)per * kb * C, g->stream));
            CCP_TRY(lex_run(g, kb, mask, g->lex_partial.p));
            hipLaunchKernelGGL(k_lex_reduce, dim3((unsigned)kb, (unsigned)C), dim3(kBlock), 0, g->stream, g->lex_partial.p, per,
                               g->lex_eps.p);
            CCP_HIP(hipGetLastError());
            CCP_HIP(hipMemcpyAsync(eps_host, g->lex_eps.p, sizeof(double) * kb * C, hipMemcpyDeviceToHost, g->stream));
            CCP_HIP(hipStreamSynchronize(g->stream));
            // how far the rule is, in sweeps, for the channel nearest to it (the step of the batch's last sweep against
            // the one half a batch earlier)
            double nearest = 1e300;
            for (int ch = 0; ch < C && kb >= 2; ++ch) {
                if (!((mask >> ch) & 1u)) continue;
                const double e1 = eps_host[(size_t)(kb - 1) * C + ch], e0 = eps_host[(size_t)(kb / 2 - 1) * C + ch];
                double left = 1e300;
                if (!(e1 > epsilon)) left = 0.0;
                else if (e1 < e0 && epsilon > 0.0) left = std::log(epsilon / e1) / (std::log(e1 / e0) / (double)(kb - kb / 2));
                nearest = std::min(nearest, left);
            }
            if (nearest > 4.0 * batch) batch = std::min(batch * 2, batch_cap);
            for (int ch = 0; ch < C; ++ch) {
                if (!((mask >> ch) & 1u)) continue;
                int stop = -1;
                for (int k = 0; k < kb; ++k) {
                    if ((done + k + 1) % check_every != 0) continue;
                    last_eps[ch] = eps_host[(size_t)k * C + ch];
                    if (!(last_eps[ch] > epsilon)) {
                        stop = k;
                        break;
                    }
                }
                if (stop < 0) continue;
                converged[ch] = 1;
                iterations_of[ch] = done + stop + 1;
                mask &= ~(1u << ch);
                if (stop < kb - 1) {
                    // the pipeline ran past the sweep the rule stops at: redo exactly stop+1 sweeps of
                    // this channel from the snapshot taken before the batch
                    CCP_HIP(hipMemcpyAsync(lex_xd(g) + (size_t)ch * lg.plane, g->lex_snap.p + (size_t)ch * lg.plane,
                                           (size_t)lg.plane * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
                    CCP_TRY(lex_run(g, stop + 1, 1u << ch, nullptr));
                }
            }
            done += kb;
        }
        for (int ch = 0; ch < C; ++ch)
            if (!converged[ch]) iterations_of[ch] = done;
    }
    hipLaunchKernelGGL((k_lex_convert_tiled<false>), tgrid, dim3(kBlock), 0, g->stream, g->x.p, lex_xd(g), g->geom, lg);
    CCP_HIP(hipGetLastError());
    return finish_solve(g, report, [&](int ch, ccp_gs_report &r) {
        r.converged = converged[ch];
        r.iterations = iterations_of[ch];
        r.last_l1_step = last_eps[ch];
    });
} CCP_ABI_CATCH

int ccp_debug_lex_tickets(int32_t width, int32_t depth, int32_t groups, uint32_t *order, int64_t capacity, int32_t *strips, int64_t *count)
try {
    if (width < 1 || groups < 1 || (depth != 1 && depth != 2 && depth != 4 && depth != 8) || (long)groups * depth > kLexLaunchSweeps || !strips || !count)
        return CCP_ERR_BAD_ARG;
    std::vector<unsigned> t;
    lex_ticket_order(width, depth, groups, t);
    *strips = lex_strip_count(width, depth, groups);
    *count = (int64_t)t.size();
    if (order) {
        if (capacity < (int64_t)t.size()) return CCP_ERR_BAD_ARG;
        std::copy(t.begin(), t.end(), order);
    }
    return CCP_OK;
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
        CCP_TRY(weighted_apply<1>(g));
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

// ============================================================================================
// Image I/O and assembly (include/ccp_gs.h): every image-shaped input or output is read through a strided view
// (ccp_grid_io.hpp).  The ccp_grid_*_device calls pass views of the caller's device arrays; nothing is staged,
// allocated or waited for.  Their host twins stage into device memory, launch the same kernels on views of the
// staging buffers, and wait.
// ============================================================================================
namespace {

int check_view(const ccp_grid *g, const ccp_device_array *a, unsigned dtypes, bool output, long n, long y, long x, long c)
{
    return check_view_on(g->desc.device, a, dtypes, output, n, y, x, c);
}

template <typename T>
View<T> view_of(const ccp_device_array *a)
{
    return View<T>{static_cast<T *>(const_cast<void *>(a->data)), (long)a->stride_n, (long)a->stride_y, (long)a->stride_x,
                   (long)a->stride_c};
}

// Which gather / scatter form a view of W x C rows allows: the vector forms need every pair 2-element aligned.
int io_kind(const ccp_device_array *a, int C)
{
    const size_t es = dtype_bytes(a->dtype);
    const bool rows_even = a->stride_y % 2 == 0 && (uintptr_t)a->data % (2 * es) == 0;
    if (C == 3 && a->stride_c == 1 && a->stride_x == 3 && rows_even) return kRgb;
    if (a->stride_x == 1 && rows_even && (C == 1 || a->stride_c % 2 == 0)) return kPairs;
    return kGeneral;
}

int io_rows(const ccp_grid *g, int first_row, int n_rows)
{
    if (n_rows < 0 || first_row < g->geom.y0 || (long)first_row + n_rows > (long)g->geom.y0 + g->geom.local_rows) return CCP_ERR_BAD_ARG;
    return CCP_OK;
}

dim3 io_grid(const ccp_grid *g, int n_rows) { return dim3((unsigned)(((g->desc.width + 1) / 2 + kBlock - 1) / kBlock), (unsigned)n_rows); }

template <typename T, bool MASKED>
int launch_scatter(ccp_grid *g, double *dst, const ccp_device_array *a, int first_row, int n_rows)
{
    const View<const T> v = view_of<const T>(a);
    const int C = g->desc.channels;
    const dim3 grid = io_grid(g, n_rows);
    switch (io_kind(a, C)) {
    case kRgb:
        hipLaunchKernelGGL((k_io_scatter<kRgb, MASKED, T>), grid, dim3(kBlock), 0, g->stream, dst, v, g->maskp.p, g->geom, first_row, C);
        break;
    case kPairs:
        hipLaunchKernelGGL((k_io_scatter<kPairs, MASKED, T>), grid, dim3(kBlock), 0, g->stream, dst, v, g->maskp.p, g->geom, first_row, C);
        break;
    default:
        hipLaunchKernelGGL((k_io_scatter<kGeneral, MASKED, T>), grid, dim3(kBlock), 0, g->stream, dst, v, g->maskp.p, g->geom, first_row, C);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

template <typename T>
int launch_gather(ccp_grid *g, const double *src, const ccp_device_array *a, int first_row, int n_rows)
{
    const View<T> v = view_of<T>(a);
    const int C = g->desc.channels;
    const dim3 grid = io_grid(g, n_rows);
    switch (io_kind(a, C)) {
    case kRgb:
        hipLaunchKernelGGL((k_io_gather<kRgb, T>), grid, dim3(kBlock), 0, g->stream, src, v, g->geom, first_row, C);
        break;
    case kPairs:
        hipLaunchKernelGGL((k_io_gather<kPairs, T>), grid, dim3(kBlock), 0, g->stream, src, v, g->geom, first_row, C);
        break;
    default:
        hipLaunchKernelGGL((k_io_gather<kGeneral, T>), grid, dim3(kBlock), 0, g->stream, src, v, g->geom, first_row, C);
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

constexpr unsigned kF32F64 = (1u << CCP_DTYPE_F32) | (1u << CCP_DTYPE_F64);
constexpr unsigned kF32 = 1u << CCP_DTYPE_F32;
constexpr unsigned kU8 = 1u << CCP_DTYPE_U8;

int set_device(ccp_grid *g, double *dst, const ccp_device_array *a, int first_row, int n_rows)
{
    CCP_TRY(bind(g));
    CCP_TRY(io_rows(g, first_row, n_rows));
    CCP_TRY(check_view(g, a, kF32F64, false, 1, n_rows, g->desc.width, g->desc.channels));
    if (n_rows == 0) return edge_timeout_status(g);
    int st;
    if (a->dtype == CCP_DTYPE_F64)
        st = g->masked ? launch_scatter<double, true>(g, dst, a, first_row, n_rows) : launch_scatter<double, false>(g, dst, a, first_row, n_rows);
    else
        st = g->masked ? launch_scatter<float, true>(g, dst, a, first_row, n_rows) : launch_scatter<float, false>(g, dst, a, first_row, n_rows);
    CCP_TRY(st);
    return edge_timeout_status(g);
}

int get_device(ccp_grid *g, const double *src, const ccp_device_array *a, int first_row, int n_rows)
{
    CCP_TRY(bind(g));
    CCP_TRY(io_rows(g, first_row, n_rows));
    CCP_TRY(check_view(g, a, kF32F64, true, 1, n_rows, g->desc.width, g->desc.channels));
    if (n_rows == 0) return edge_timeout_status(g);
    CCP_TRY(a->dtype == CCP_DTYPE_F64 ? launch_gather<double>(g, src, a, first_row, n_rows) : launch_gather<float>(g, src, a, first_row, n_rows));
    return edge_timeout_status(g);
}

bool single_block(const ccp_grid *g) { return !(g->ghost_top || g->ghost_bottom || g->desc.row_count != g->desc.height); }

int weighted_handle(ccp_grid *g)
{
    CCP_TRY(bind(g));
    return g->weighted ? CCP_OK : CCP_ERR_UNSUPPORTED;
}

// Rows [ya, yb) of an interleaved host image (W x C elements of T per row, `stride` bytes apart) into a packed
// device buffer, asynchronously on the handle's stream.
template <typename T>
int upload_window(ccp_grid *g, DevBuf<T> &dev, const T *host, int64_t stride, int ya, int yb)
{
    const size_t row = (size_t)g->desc.width * g->desc.channels * sizeof(T);
    CCP_TRY(dev.alloc((size_t)(yb - ya) * g->desc.width * g->desc.channels));
    CCP_HIP(hipMemcpy2DAsync(dev.p, row, reinterpret_cast<const char *>(host) + (size_t)ya * (size_t)stride, (size_t)stride,
                             row, (size_t)(yb - ya), hipMemcpyHostToDevice, g->stream));
    return CCP_OK;
}

// A packed staging buffer of the host entry points as the view the kernels read: interleaved W x C rows of a row
// window that starts at image row `ya` (the images of a stack `plane` elements apart).  Views are indexed by IMAGE
// row, so the base is moved back by `ya` rows here on the host; a kernel only touches the rows its window covers
// (blend_window below, the owned rows for the composite), so nothing in front of `p` is ever dereferenced.
template <typename T>
View<T> staged_view(T *p, int W, int C, int ya = 0, long plane = 0)
{
    const long row = (long)W * C;
    return View<T>{p - (long)ya * row, plane, row, (long)C, 1};
}

BlendMask blend_mask(const ccp_grid *g) { return BlendMask{g->maskp.p, g->mask_edge.p, g->geom}; }

// the image rows the assembly reads: the local rows and one row above and below where they exist
void blend_window(const ccp_grid *g, int *ya, int *yb)
{
    *ya = std::max(0, g->geom.y0 - 1);
    *yb = std::min(g->geom.H, g->geom.y0 + g->geom.local_rows + 1);
}

// Does the region touch the canvas's outer rows or columns?  Known from ccp_grid_set_mask_host; after the device
// twin (whole-canvas handles only) read back once from the split mask.
int blend_border(ccp_grid *g, bool *touches)
{
    if (g->mask_border < 0) {
        if (!g->mask_edge_known) return CCP_ERR_STATE;
        const Geom &geo = g->geom;
        std::vector<unsigned char> split((size_t)geo.ch_stride);
        CCP_HIP(hipMemcpyAsync(split.data(), g->maskp.p, split.size(), hipMemcpyDeviceToHost, g->stream));
        CCP_HIP(hipStreamSynchronize(g->stream));
        auto at = [&](int y, int x) { return split[(size_t)((2L * y + ((x + y) & 1)) * geo.pitch + (x >> 1))] != 0; };
        bool border = false;
        for (int y = 0; y < geo.H && !border; ++y) {
            border = at(y, 0) || at(y, geo.W - 1);
            if (y == 0 || y == geo.H - 1)
                for (int x = 0; x < geo.W && !border; ++x) border = at(y, x);
        }
        g->mask_border = border ? 1 : 0;
    }
    *touches = g->mask_border != 0;
    return CCP_OK;
}

// ---- one launcher per operation: launch geometry, template dispatch, the launch status and the handle state the
// operation leaves behind.  The arguments are validated; the _device entry points pass the caller's views, the host
// entry points the views of what they staged.
using VF = View<const float>;
using VU = View<const uint8_t>;

// one lane per pixel of a row: ceil(W / kBlock) blocks by `rows` (by `channels` where a lane serves one channel)
dim3 pixel_grid(const ccp_grid *g, int rows, int channels = 1)
{
    return dim3((unsigned)((g->desc.width + kBlock - 1) / kBlock), (unsigned)rows, (unsigned)channels);
}

int assemble_rhs(ccp_grid *g, const VF &gx, const VF &gy, const int32_t *constraint)
{
    const int C = g->desc.channels;
    Pins pins{};
    for (int ch = 0; ch < C; ++ch) pins.v[ch] = constraint[ch];
    hipLaunchKernelGGL((k_assemble_rhs<VF, Pins>), pixel_grid(g, g->desc.height, C), dim3(kBlock), 0, g->stream, g->b.p, g->geom, gx, gy, pins);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int assemble_from_images(ccp_grid *g, const VU &images, const VU &label, bool init_x)
{
    const dim3 grid = pixel_grid(g, g->desc.height, 3);
    if (init_x)
        hipLaunchKernelGGL((k_assemble_from_images<true, VU, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, g->geom, images, label);
    else
        hipLaunchKernelGGL((k_assemble_from_images<false, VU, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, g->geom, images, label);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int store_u8(ccp_grid *g, const View<uint8_t> &out)
{
    hipLaunchKernelGGL((k_store_u8<View<uint8_t>>), pixel_grid(g, g->desc.height, g->desc.channels), dim3(kBlock), 0, g->stream, g->x.p,
                       g->geom, out);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int load_u8(ccp_grid *g, const VU &image)
{
    hipLaunchKernelGGL((k_load_u8<VU>), pixel_grid(g, g->desc.height, g->desc.channels), dim3(kBlock), 0, g->stream, g->x.p, g->geom, image);
    CCP_HIP(hipGetLastError());
    return zero_unmasked(g, g->x.p);
}

int blend_field_rhs(ccp_grid *g, const VF &gx, const VF &gy, const VU &canvas, bool init_x)
{
    const dim3 grid = pixel_grid(g, g->geom.local_rows);
    const int C = g->desc.channels;
    if (init_x)
        hipLaunchKernelGGL((k_blend_field_rhs<true, VF, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, blend_mask(g), gx, gy, canvas, C);
    else
        hipLaunchKernelGGL((k_blend_field_rhs<false, VF, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, blend_mask(g), gx, gy, canvas, C);
    CCP_HIP(hipGetLastError());
    if (init_x) g->half_sweeps_since_refresh = 0;         // x is exact on every local row
    return CCP_OK;
}

int blend_clone_rhs(ccp_grid *g, const VU &source, const VU &target, int mode, int init)
{
    const dim3 grid = pixel_grid(g, g->geom.local_rows);
    const int C = g->desc.channels;
    if (mode == CCP_CLONE_MIXED)
        hipLaunchKernelGGL((k_blend_clone_rhs<true, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, blend_mask(g), source, target, C, init);
    else
        hipLaunchKernelGGL((k_blend_clone_rhs<false, VU>), grid, dim3(kBlock), 0, g->stream, g->b.p, g->x.p, blend_mask(g), source, target, C, init);
    CCP_HIP(hipGetLastError());
    if (init) g->half_sweeps_since_refresh = 0;
    return CCP_OK;
}

int blend_composite(ccp_grid *g, const VU &canvas, const View<uint8_t> &out)
{
    hipLaunchKernelGGL((k_blend_composite<VU, View<uint8_t>>), pixel_grid(g, g->desc.row_count), dim3(kBlock), 0, g->stream, g->x.p,
                       blend_mask(g), canvas, out, g->desc.channels);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// a caller's view (or none) as the weighted handle's operator kernels read it
ImageView image_view(const ccp_device_array *a, double dflt)
{
    if (!a) return ImageView{nullptr, 0, 0, 0, 0, dflt};
    return ImageView{a->data, (long)a->stride_y, (long)a->stride_x, (long)a->stride_c, a->dtype, dflt};
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

}  // namespace

extern "C" {

int ccp_grid_set_b_device(ccp_grid *g, const ccp_device_array *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return set_device(g, g->b.p, rows, first_row, n_rows);
} CCP_ABI_CATCH

int ccp_grid_set_x_device(ccp_grid *g, const ccp_device_array *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return set_device(g, g->x.p, rows, first_row, n_rows);
} CCP_ABI_CATCH

int ccp_grid_get_x_device(ccp_grid *g, const ccp_device_array *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return get_device(g, g->x.p, rows, first_row, n_rows);
} CCP_ABI_CATCH

int ccp_grid_get_b_device(ccp_grid *g, const ccp_device_array *rows, int32_t first_row, int32_t n_rows)
try {
    if (!g) return CCP_ERR_BAD_ARG;
    return get_device(g, g->b.p, rows, first_row, n_rows);
} CCP_ABI_CATCH

// ---- the image-shaped entry points in pairs: the host form stages into device memory, calls the launcher its
// _device twin calls on the caller's arrays, and waits; the twin enqueues and returns.  Each keeps its own order of
// refusals.

int ccp_grid_assemble_rhs(ccp_grid *g, const float *gx, const float *gy, int64_t row_stride_bytes, const int32_t *constraint)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!gx || !gy || !constraint) return CCP_ERR_BAD_ARG;
    if (g->masked) return CCP_ERR_UNSUPPORTED;            // SolveChannel's right-hand side belongs to SolveChannel's matrix
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    const size_t row_bytes = (size_t)W * C * sizeof(float);
    if (row_stride_bytes < (int64_t)row_bytes) return CCP_ERR_BAD_ARG;
    DevBuf<float> dgx, dgy;
    CCP_TRY(dgx.alloc((size_t)W * H * C));
    CCP_TRY(dgy.alloc((size_t)W * H * C));
    // only rows y < H-1 and columns x < W-1 are defined in the reference (PhotoMontage.cpp:416-425);
    // the kernel never reads the rest, but the copy must not touch it on the host either.
    const size_t copy_rows = H > 1 ? (size_t)(H - 1) : 0;
    CCP_HIP(hipMemsetAsync(dgx.p, 0, (size_t)W * H * C * sizeof(float), g->stream));
    CCP_HIP(hipMemsetAsync(dgy.p, 0, (size_t)W * H * C * sizeof(float), g->stream));
    if (copy_rows && W > 1) {
        const size_t width_bytes = (size_t)(W - 1) * C * sizeof(float);
        CCP_HIP(hipMemcpy2DAsync(dgx.p, row_bytes, gx, (size_t)row_stride_bytes, width_bytes, copy_rows, hipMemcpyHostToDevice, g->stream));
        CCP_HIP(hipMemcpy2DAsync(dgy.p, row_bytes, gy, (size_t)row_stride_bytes, width_bytes, copy_rows, hipMemcpyHostToDevice, g->stream));
    }
    CCP_TRY(assemble_rhs(g, staged_view<const float>(dgx.p, W, C), staged_view<const float>(dgy.p, W, C), constraint));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_assemble_rhs_device(ccp_grid *g, const ccp_device_array *gx, const ccp_device_array *gy, const int32_t *constraint)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!gx || !gy || !constraint) return CCP_ERR_BAD_ARG;
    if (g->masked) return CCP_ERR_UNSUPPORTED;
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    CCP_TRY(check_view(g, gx, kF32, false, 1, H, W, C));
    CCP_TRY(check_view(g, gy, kF32, false, 1, H, W, C));
    return assemble_rhs(g, view_of<const float>(gx), view_of<const float>(gy), constraint);
} CCP_ABI_CATCH

int ccp_grid_assemble_from_images(ccp_grid *g, const uint8_t *const *images, int32_t n_images,
                                  int64_t image_stride_bytes, const uint8_t *label, int64_t label_stride_bytes,
                                  int32_t init_x_from_composite)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!images || !label || n_images < 1 || n_images > 256) return CCP_ERR_BAD_ARG;
    if (g->desc.channels != 3 || g->masked) return CCP_ERR_UNSUPPORTED;      // BGR images; SolveChannel's matrix
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height;
    if (image_stride_bytes < (int64_t)W * 3 || label_stride_bytes < W) return CCP_ERR_BAD_ARG;
    for (int k = 0; k < n_images; ++k)
        if (!images[k]) return CCP_ERR_BAD_ARG;
    // labels must select existing images (the reference indexes Images[label] unchecked)
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (label[(size_t)y * label_stride_bytes + x] >= n_images) return CCP_ERR_BAD_ARG;
    DevBuf<uint8_t> dimg, dlab;
    const size_t plane = (size_t)W * H * 3;
    CCP_TRY(dimg.alloc(plane * n_images));
    CCP_TRY(dlab.alloc((size_t)W * H));
    for (int k = 0; k < n_images; ++k)
        CCP_HIP(hipMemcpy2DAsync(dimg.p + plane * k, (size_t)W * 3, images[k], (size_t)image_stride_bytes, (size_t)W * 3,
                                 (size_t)H, hipMemcpyHostToDevice, g->stream));
    CCP_HIP(hipMemcpy2DAsync(dlab.p, (size_t)W, label, (size_t)label_stride_bytes, (size_t)W, (size_t)H,
                             hipMemcpyHostToDevice, g->stream));
    CCP_TRY(assemble_from_images(g, staged_view<const uint8_t>(dimg.p, W, 3, 0, (long)plane), staged_view<const uint8_t>(dlab.p, W, 1),
                                 init_x_from_composite != 0));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_assemble_from_images_device(ccp_grid *g, const ccp_device_array *images, int32_t n_images,
                                         const ccp_device_array *label, int32_t init_x_from_composite)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!images || !label || n_images < 1 || n_images > 256) return CCP_ERR_BAD_ARG;
    if (g->desc.channels != 3 || g->masked) return CCP_ERR_UNSUPPORTED;
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height;
    CCP_TRY(check_view(g, images, kU8, false, n_images, H, W, 3));
    CCP_TRY(check_view(g, label, kU8, false, 1, H, W, 1));
    const VU lab = view_of<const uint8_t>(label);
    // labels must select existing images: checked on the device before any image is read
    unsigned bad = 0;
    CCP_HIP(hipMemsetAsync(g->io_bad.p, 0, sizeof(unsigned), g->stream));
    const long blocks = std::min<long>(2048, ((long)W * H + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_io_label_check, dim3((unsigned)blocks), dim3(kBlock), 0, g->stream, lab, W, H, (int)n_images, g->io_bad.p);
    CCP_HIP(hipGetLastError());
    CCP_HIP(hipMemcpyAsync(&bad, g->io_bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    if (bad) return CCP_ERR_BAD_ARG;
    return assemble_from_images(g, view_of<const uint8_t>(images), lab, init_x_from_composite != 0);
} CCP_ABI_CATCH

int ccp_grid_store_u8(ccp_grid *g, uint8_t *out, int64_t row_stride_bytes)
try {
    CCP_TRY(bind(g));
    if (!out) return CCP_ERR_BAD_ARG;
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    if (row_stride_bytes < (int64_t)W * C) return CCP_ERR_BAD_ARG;
    DevBuf<uint8_t> d;
    CCP_TRY(d.alloc((size_t)W * H * C));
    CCP_TRY(store_u8(g, staged_view(d.p, W, C)));
    CCP_HIP(hipMemcpy2DAsync(out, (size_t)row_stride_bytes, d.p, (size_t)W * C, (size_t)W * C, (size_t)H, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_store_u8_device(ccp_grid *g, const ccp_device_array *out)
try {
    CCP_TRY(bind(g));
    if (!out) return CCP_ERR_BAD_ARG;
    if (!single_block(g)) return CCP_ERR_STATE;
    CCP_TRY(check_view(g, out, kU8, true, 1, g->desc.height, g->desc.width, g->desc.channels));
    return store_u8(g, view_of<uint8_t>(out));
} CCP_ABI_CATCH

int ccp_grid_set_x_u8(ccp_grid *g, const uint8_t *image, int64_t row_stride_bytes)
try {
    CCP_TRY(bind(g));
    if (!image) return CCP_ERR_BAD_ARG;
    if (!single_block(g)) return CCP_ERR_STATE;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    if (row_stride_bytes < (int64_t)W * C) return CCP_ERR_BAD_ARG;
    DevBuf<uint8_t> d;
    CCP_TRY(upload_window(g, d, image, row_stride_bytes, 0, H));
    CCP_TRY(load_u8(g, staged_view<const uint8_t>(d.p, W, C)));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_set_x_u8_device(ccp_grid *g, const ccp_device_array *image)
try {
    CCP_TRY(bind(g));
    if (!image) return CCP_ERR_BAD_ARG;
    if (!single_block(g)) return CCP_ERR_STATE;
    CCP_TRY(check_view(g, image, kU8, false, 1, g->desc.height, g->desc.width, g->desc.channels));
    return load_u8(g, view_of<const uint8_t>(image));
} CCP_ABI_CATCH

int ccp_grid_assemble_region_rhs(ccp_grid *g, const float *gx, const float *gy, int64_t field_stride_bytes,
                                 const uint8_t *canvas, int64_t canvas_stride_bytes, int32_t init_x_from_canvas)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!gx || !gy || !canvas) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, C = g->desc.channels;
    if (field_stride_bytes < (int64_t)W * C * (int64_t)sizeof(float) || canvas_stride_bytes < (int64_t)W * C) return CCP_ERR_BAD_ARG;
    if (!g->masked) return CCP_ERR_UNSUPPORTED;           // SolveChannel's matrix has its own assembly
    if (!g->mask_edge_known) return CCP_ERR_STATE;
    int ya, yb;
    blend_window(g, &ya, &yb);
    DevBuf<float> dgx, dgy;
    DevBuf<uint8_t> dcan;
    CCP_TRY(upload_window(g, dgx, gx, field_stride_bytes, ya, yb));
    CCP_TRY(upload_window(g, dgy, gy, field_stride_bytes, ya, yb));
    CCP_TRY(upload_window(g, dcan, canvas, canvas_stride_bytes, ya, yb));
    CCP_TRY(blend_field_rhs(g, staged_view<const float>(dgx.p, W, C, ya), staged_view<const float>(dgy.p, W, C, ya),
                            staged_view<const uint8_t>(dcan.p, W, C, ya), init_x_from_canvas != 0));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_assemble_region_rhs_device(ccp_grid *g, const ccp_device_array *gx, const ccp_device_array *gy,
                                        const ccp_device_array *canvas, int32_t init_x_from_canvas)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!gx || !gy || !canvas) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    CCP_TRY(check_view(g, gx, kF32, false, 1, H, W, C));
    CCP_TRY(check_view(g, gy, kF32, false, 1, H, W, C));
    CCP_TRY(check_view(g, canvas, kU8, false, 1, H, W, C));
    if (!g->masked) return CCP_ERR_UNSUPPORTED;
    if (!g->mask_edge_known) return CCP_ERR_STATE;
    return blend_field_rhs(g, view_of<const float>(gx), view_of<const float>(gy), view_of<const uint8_t>(canvas), init_x_from_canvas != 0);
} CCP_ABI_CATCH

int ccp_grid_assemble_clone(ccp_grid *g, const uint8_t *source, int64_t source_stride_bytes, const uint8_t *target,
                            int64_t target_stride_bytes, int32_t mode, int32_t init)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!source || !target) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, C = g->desc.channels;
    if (source_stride_bytes < (int64_t)W * C || target_stride_bytes < (int64_t)W * C) return CCP_ERR_BAD_ARG;
    if ((mode != CCP_CLONE_IMPORT && mode != CCP_CLONE_MIXED) || init < 0 || init > 2) return CCP_ERR_BAD_ARG;
    if (!g->masked) return CCP_ERR_UNSUPPORTED;
    if (!g->mask_edge_known) return CCP_ERR_STATE;
    bool touches = false;
    CCP_TRY(blend_border(g, &touches));
    if (touches) return CCP_ERR_UNSUPPORTED;              // the diagonal is 4 everywhere: no neighbour may be missing
    int ya, yb;
    blend_window(g, &ya, &yb);
    DevBuf<uint8_t> dsrc, dtgt;
    CCP_TRY(upload_window(g, dsrc, source, source_stride_bytes, ya, yb));
    CCP_TRY(upload_window(g, dtgt, target, target_stride_bytes, ya, yb));
    CCP_TRY(blend_clone_rhs(g, staged_view<const uint8_t>(dsrc.p, W, C, ya), staged_view<const uint8_t>(dtgt.p, W, C, ya), mode, init));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_grid_assemble_clone_device(ccp_grid *g, const ccp_device_array *source, const ccp_device_array *target, int32_t mode,
                                   int32_t init)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!source || !target) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    CCP_TRY(check_view(g, source, kU8, false, 1, H, W, C));
    CCP_TRY(check_view(g, target, kU8, false, 1, H, W, C));
    if ((mode != CCP_CLONE_IMPORT && mode != CCP_CLONE_MIXED) || init < 0 || init > 2) return CCP_ERR_BAD_ARG;
    if (!g->masked) return CCP_ERR_UNSUPPORTED;
    if (!g->mask_edge_known) return CCP_ERR_STATE;
    bool touches = false;
    CCP_TRY(blend_border(g, &touches));
    if (touches) return CCP_ERR_UNSUPPORTED;
    return blend_clone_rhs(g, view_of<const uint8_t>(source), view_of<const uint8_t>(target), mode, init);
} CCP_ABI_CATCH

int ccp_grid_store_u8_composite(ccp_grid *g, const uint8_t *canvas, int64_t canvas_stride_bytes, uint8_t *out,
                                int64_t out_stride_bytes)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!canvas || !out) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, C = g->desc.channels;
    if (canvas_stride_bytes < (int64_t)W * C || out_stride_bytes < (int64_t)W * C) return CCP_ERR_BAD_ARG;
    if (!g->masked) return CCP_ERR_UNSUPPORTED;
    const int y_lo = g->desc.row_begin, rows = g->desc.row_count;
    DevBuf<uint8_t> dcan, dout;
    CCP_TRY(upload_window(g, dcan, canvas, canvas_stride_bytes, y_lo, y_lo + rows));
    CCP_TRY(dout.alloc((size_t)rows * W * C));
    CCP_TRY(blend_composite(g, staged_view<const uint8_t>(dcan.p, W, C, y_lo), staged_view(dout.p, W, C, y_lo)));
    CCP_HIP(hipMemcpy2DAsync(out + (size_t)y_lo * (size_t)out_stride_bytes, (size_t)out_stride_bytes, dout.p, (size_t)W * C,
                             (size_t)W * C, (size_t)rows, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));
    return edge_timeout_status(g);
} CCP_ABI_CATCH

int ccp_grid_store_u8_composite_device(ccp_grid *g, const ccp_device_array *canvas, const ccp_device_array *out)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!canvas || !out) return CCP_ERR_BAD_ARG;
    const int W = g->desc.width, H = g->desc.height, C = g->desc.channels;
    CCP_TRY(check_view(g, canvas, kU8, false, 1, H, W, C));
    CCP_TRY(check_view(g, out, kU8, true, 1, H, W, C));
    if (!g->masked) return CCP_ERR_UNSUPPORTED;
    CCP_TRY(blend_composite(g, view_of<const uint8_t>(canvas), view_of<uint8_t>(out)));
    return edge_timeout_status(g);
} CCP_ABI_CATCH

int ccp_grid_set_mask_device(ccp_grid *g, const ccp_device_array *mask)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (!g->masked) return CCP_ERR_STATE;
    CCP_TRY(check_view(g, mask, kF32F64 | kU8, false, 1, g->desc.height, g->desc.width, 1));
    const Geom &geo = g->geom;
    const dim3 grid((unsigned)((geo.pitch + kBlock - 1) / kBlock), (unsigned)geo.local_rows + 4);
    CCP_HIP(hipMemsetAsync(g->mask_counters.p, 0, 2 * sizeof(unsigned long long), g->stream));
    switch (mask->dtype) {
    case CCP_DTYPE_U8:
        hipLaunchKernelGGL(k_mask_split<uint8_t>, grid, dim3(kBlock), 0, g->stream, view_of<const uint8_t>(mask), g->maskp.p, g->mask_edge.p, geo,
                           g->mask_counters.p);
        break;
    case CCP_DTYPE_F32:
        hipLaunchKernelGGL(k_mask_split<float>, grid, dim3(kBlock), 0, g->stream, view_of<const float>(mask), g->maskp.p, g->mask_edge.p, geo,
                           g->mask_counters.p);
        break;
    default:
        hipLaunchKernelGGL(k_mask_split<double>, grid, dim3(kBlock), 0, g->stream, view_of<const double>(mask), g->maskp.p, g->mask_edge.p, geo,
                           g->mask_counters.p);
    }
    CCP_HIP(hipGetLastError());
    unsigned long long counters[2] = {0, 0};
    CCP_HIP(hipMemcpyAsync(counters, g->mask_counters.p, sizeof counters, hipMemcpyDeviceToHost, g->stream));
    CCP_HIP(hipStreamSynchronize(g->stream));            // the two counters, and the caller's mask may go (as the host twin)
    g->mask_edge_known = true;
    g->mask_border = counters[1] ? 1 : 0;
    g->unknowns = (long)counters[0];
    CCP_TRY(mask_replaced(g));
    return CCP_OK;
} CCP_ABI_CATCH

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

}  // extern "C"

// ============================================================================================
// Weighted grids (include/ccp_gs.h, CCP_GRID_WEIGHTED; kernels: ccp_grid_weighted.hpp)
// ============================================================================================
namespace {

// a new operator is coming: the old one, its counts and the hierarchy built on it go
void drop_operator(ccp_grid *g)
{
    mg_release(&g->mg);
    g->has_op = g->has_fixed = false;
    g->per_channel = false;
    g->mg_nullspace.forget();
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
// way: a refusal leaves the handle with none.  The three extra planes stay only if some set has a fixed pixel: with
// none the four planes are what the call without a mask forms, bit for bit.
int form_operator(ccp_grid *g, bool per_channel, const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView *fixed)
{
    const Geom &geo = g->geom;
    const long n = geo.ch_stride;
    const int sets = per_channel ? g->desc.channels : 1;
    drop_operator(g);
    g->wcons.release();
    CCP_TRY(operator_planes(g, sets));
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
    if (count[0] || !any_fixed) g->wcons.release();
    if (count[0]) return CCP_ERR_BAD_ARG;
    for (int c = 0; c < sets; ++c) {
        g->pc_fixed[c] = fixed ? (long)count[1 + 3 * c] : 0;
        g->pc_live[c] = fixed ? (long)geo.W * geo.H - (long)count[1 + 3 * c] - (long)count[2 + 3 * c] : -1;
        g->pc_edges[c] = fixed ? (long)count[3 + 3 * c] : 0;
    }
    g->has_op = true;
    g->per_channel = per_channel;
    g->has_fixed = any_fixed;
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

// ccp_grid_set_weights_[constrained_]device and ccp_grid_set_weights_per_channel_device: the views are H x W for the
// shared operator and H x W x channels for one operator per channel
int set_weights_device(ccp_grid *g, bool per_channel, const ccp_device_array *wx, const ccp_device_array *wy, const ccp_device_array *lambda,
                       const ccp_device_array *fixed)
{
    CCP_TRY(weighted_handle(g));
    const int W = g->desc.width, H = g->desc.height, C = per_channel ? g->desc.channels : 1;
    const ccp_device_array *src[3] = {wx, wy, lambda};
    const double dflt[3] = {1.0, 1.0, 0.0};
    ImageView v[3];
    for (int i = 0; i < 3; ++i) {
        if (src[i]) CCP_TRY(check_view(g, src[i], kF32F64, false, 1, H, W, C));
        v[i] = image_view(src[i], dflt[i]);
    }
    if (!fixed) return form_operator(g, per_channel, v[0], v[1], v[2], nullptr);
    CCP_TRY(check_view(g, fixed, kF32F64 | kU8, false, 1, H, W, C));
    const ImageView m = image_view(fixed, 0.0);
    return form_operator(g, per_channel, v[0], v[1], v[2], &m);
}

}  // namespace

extern "C" {

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
