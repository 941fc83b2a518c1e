// ccp_grid_handle.hpp — struct ccp_grid, the handle behind the ccp_grid_* calls of include/ccp_gs.h, and the few host
// helpers that more than one of its translation units needs (ccp_grid.hip: life cycle, red-black passes, solves;
// ccp_grid_lex.hip: the reference's order; ccp_grid_io.hip: I/O, assembly, blends, masks; ccp_grid_weighted.hip: weighted
// handles).  Library-internal and host-only: no kernel is defined here or in anything this header includes.
// ccp_grid_mg.hip does not include it: GridMgView / GridMgSlot (ccp_grid_mg_view.hpp) stay the multigrid's window.
#pragma once

#include "ccp_common.hpp"
#include "ccp_grid_geom.hpp"
#include "ccp_grid_mg_view.hpp"    // MgConfig, MgNullspace, MgHierarchy
#include "ccp_grid_types.hpp"      // SolveState, LexGeom, kFusedMaxT, kFusedMaxCheckedT
#include "ccp_view.hpp"

#include <algorithm>
#include <vector>

// struct ccp_grid is the C ABI's opaque type and so lives outside namespace ccp, whose types it is made of; every
// translation unit that includes this header is one of the handle's own and says the same itself.
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
    // while the operator has any or the handle reserves them (has_fixed: the planes exist), and is released otherwise.
    // wcount: the formation pass's verdict and counts
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
    // ccp_grid_refresh_weights_device (made with the handle: the refresh allocates nothing).  rcount: the refresh pass's
    // verdict and counts in wcount's layout, which stay on the device and are read whenever ccp_grid_constraint_info asks
    // while `refreshed` (the last change of the operator was a refresh; a setter clears it); op_status: the CCP_OPERATOR_*
    // word of the last refresh, 0 from the handle's creation and again after a setter, so that the enqueue solve can read it
    // on every handle: neither may depend on what the host knew when a graph was recorded, a replayed refresh moves both.
    DevBuf<unsigned long long> rcount;
    DevBuf<unsigned> op_status;
    bool refreshed = false;
    // ccp_grid_reserve_constraints / ccp_grid_refresh_constrained_device.  reserve_cons: the setters keep wcons whether or
    // not a pixel is fixed (has_fixed then says "the three planes exist", which is all its readers ask).  The fixed set a
    // constrained refresh installs is counted into words of its own, rcount[kRefreshFixedAt + k] for set k, which only that
    // call clears and counts into (a value refresh clears rcount[1 + 3 k] and does not recount it); fixed_on_device: those
    // words, not pc_fixed, hold the fixed counts -- from the first constrained refresh until a setter.
    bool reserve_cons = false;
    bool fixed_on_device = false;
    MgConfig mg_cfg;                           // ccp_grid_mg_set_* (ccp_grid_mg_view.hpp)
    MgNullspace mg_nullspace;                  // goes with the operator (drop_operator)
};

namespace ccp {

// rcount: wcount's 1 + 3 sets words of up to kMaxChannels sets, then one fixed-pixel count per set
constexpr int kRefreshFixedAt = 1 + 3 * kMaxChannels;
constexpr int kRefreshCounts = kRefreshFixedAt + kMaxChannels;

// The weighted product's launch geometry: ccp_grid.hip sizes wpart by it and reduces what ccp_grid_weighted.hip launched
constexpr int kWeightedApplyBlocks = 1024;   // blocks per (channel, colour) of k_weighted_apply

// k_weighted_apply: up to kWeightedApplyBlocks blocks per (channel, colour) striding over the colour's cells
inline dim3 weighted_apply_grid(const ccp_grid *g)
{
    const long cells = (long)g->geom.H * ((g->geom.W + 1) / 2);
    return dim3((unsigned)std::max<long>(1, std::min<long>(kWeightedApplyBlocks, (cells + kBlock - 1) / kBlock)), 1, 2 * (unsigned)g->desc.channels);
}

// ---- defined in ccp_grid.hip ---------------------------------------------------------------------------------------------
// Did a polling kernel give up on the edge flag (see ccp_grid::edge_timeout)?
int edge_timeout_status(const ccp_grid *g);
// null check, hipSetDevice, edge_timeout_status: how every entry point begins
int bind(ccp_grid *g);
// the calls a weighted handle refuses begin with this: CCP_ERR_UNSUPPORTED on one
int not_weighted(const ccp_grid *g);
// Dirichlet-mask grids: plane := 0 outside the region (all channels; a no-op on other handles)
int zero_unmasked(ccp_grid *g, double *plane);
// the events around a timed call (ccp_grid_last_timing)
int begin_timing(ccp_grid *g);
int end_timing(ccp_grid *g);

// ---- defined in ccp_grid_io.hip ------------------------------------------------------------------------------------------
// a caller's device array against the handle's device, the dtypes allowed (a mask of 1 << CCP_DTYPE_*) and the extents
// n, y, x, c (ccp_view_check.hpp)
constexpr unsigned kF32F64 = (1u << CCP_DTYPE_F32) | (1u << CCP_DTYPE_F64);
constexpr unsigned kF32 = 1u << CCP_DTYPE_F32;
constexpr unsigned kU8 = 1u << CCP_DTYPE_U8;
int check_view(const ccp_grid *g, const ccp_device_array *a, unsigned dtypes, bool output, long n, long y, long x, long c);
// a caller's view (or none) as the weighted handle's operator kernels read it
ImageView image_view(const ccp_device_array *a, double dflt);
// one lane per pixel of a row: ceil(W / kBlock) blocks by `rows` (by `channels` where a lane serves one channel)
dim3 pixel_grid(const ccp_grid *g, int rows, int channels = 1);

// ---- defined in ccp_grid_weighted.hip ------------------------------------------------------------------------------------
// b := A x (mode 0) or the residual's partial sums in wpart (mode 1) of every channel of a weighted handle
int weighted_apply(ccp_grid *g, int mode);

// ---- templates, their bodies here ----------------------------------------------------------------------------------------
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

}  // namespace ccp
