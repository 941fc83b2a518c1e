// ccp_fused_plan.hpp — how a temporally blocked red-black pass (ccp_grid_fused.hpp, ccp_grid_fused_wide.hpp) is laid out:
// chunks and strips, border and side tiles, the edge hand-off's wave count, the wide interior and its row segments, the
// launch grids; and around it the rows a pass may store after a halo refresh, the split of an iteration count into
// passes, which passes store their red halves, and the chunk heights ccp_grid_tune tries.
//
// Host-only arithmetic on plain values, no HIP: tests/cpp/fused_plan_check.cpp includes this header alone and checks it on
// the CPU.  The launchers of ccp_grid.hip copy a FusedPlan into FusedParams and launch; the kernels share the chunk and
// strip arithmetic below (CCP_FUSED_PLAN_FN), which is written against the field names FusedPlan and FusedParams have
// in common.
#pragma once

#include <algorithm>
#include <functional>
#include <vector>

#include "ccp_grid_geom.hpp"
#include "ccp_wide_plan.hpp"

#if defined(__HIPCC__)
#define CCP_FUSED_PLAN_FN __host__ __device__ __forceinline__
#define CCP_FUSED_PLAN_CONST __host__ __device__ constexpr
#else
#define CCP_FUSED_PLAN_FN inline
#define CCP_FUSED_PLAN_CONST constexpr
#endif

namespace ccp {

constexpr int kStripLanes = 64;          // half-columns per strip: one per lane of a wave
constexpr int kTileWaves = 4;            // waves (tiles) per workgroup of the pass kernels: one per SIMD
constexpr int kWideT = 8;                // the only depth built on wide strips
constexpr int kWideWaves = kTileWaves;   // waves (wide strips) per workgroup of k_fused_sweep_wide

CCP_FUSED_PLAN_CONST int fused_halo_px(int T) { return 2 * T; }               // per side
CCP_FUSED_PLAN_CONST int fused_useful_px(int T) { return 2 * kStripLanes - 4 * T; }
CCP_FUSED_PLAN_CONST int wide_useful_px(int T) { return 4 * kStripLanes - 4 * T; }
CCP_FUSED_PLAN_CONST int fused_n_strips(int W, int T) { return (W + fused_useful_px(T) - 1) / fused_useful_px(T); }

// ---- chunks: P is a FusedPlan or the kernels' FusedParams ----------------------------------------------------------
// blockIdx.y -> chunk with the edge chunks first (workgroups are dispatched in block-index order)
template <class P>
CCP_FUSED_PLAN_FN int fused_chunk_of(const P &p, int y)
{
    const int n_e = p.first_edge + p.last_edge;
    if (y < n_e) return (p.first_edge && y == 0) ? 0 : p.n_chunks - 1;
    return y - n_e + p.first_edge;
}

template <class P>
CCP_FUSED_PLAN_FN bool fused_is_edge_chunk(const P &p, int chunk)
{
    return (p.first_edge && chunk == 0) || (p.last_edge && chunk == p.n_chunks - 1);
}

// rows [ra, rb) of chunk c
template <class P>
CCP_FUSED_PLAN_FN void fused_chunk_rows(const P &p, int c, int &ra, int &rb)
{
    if (p.first_rows > 0 && c == 0) {
        ra = p.st_lo;
        rb = p.st_lo + p.first_rows;
    } else if (p.last_rows > 0 && c == p.n_chunks - 1) {
        ra = p.st_hi - p.last_rows;
        rb = p.st_hi;
    } else {
        const int k = c - (p.first_rows > 0 ? 1 : 0);
        const int end = p.st_hi - p.last_rows;
        ra = p.st_lo + p.first_rows + k * p.rows_per_chunk;
        rb = ra + p.rows_per_chunk < end ? ra + p.rows_per_chunk : end;
    }
}

// ---- what a plan is made from ---------------------------------------------------------------------------------------
struct FusedPlanInput {
    Geom g;
    bool stale_top = false, stale_bottom = false;   // the side ends in ghost rows of a neighbour block, not at the image
    int ghost = 0;                                  // ghost rows asked for: half-sweeps a refresh pays for
    int ghost_top = 0, ghost_bottom = 0;            // ghost rows the block has (clipped at the image)
    int send_up = 0, send_down = 0;                 // owned rows the upper / lower neighbour takes (0: as many as edge_rows)
    int channels = 1;
    int cus = 0;                                    // compute units: the wide pass holds kWideWaves waves on each
    int rows_per_chunk = 128;                       // the chunk height in force for this depth
    bool short_edges = true;                        // chunk rows at an image edge are short
    bool all_border = false;                        // debug: every tile through the border launch
    int side_rows_override = 0;
    bool wide = true;                               // depth-8 unchecked passes run their ordinary tiles on wide strips
    int wide_segments = -1;                         // -1 the planner (ccp_wide_plan.hpp), 0 the interior chunks, n > 0: n segments
};

struct FusedPassKind {
    int T = 1;
    int st_lo = 0, st_hi = 0;   // local rows the pass finalises and stores
    int l1 = 0;                 // 0 unchecked, 1 step of the last sweep, 2 step of every sweep
    int edge_rows = 0;          // > 0: an edge pass that signals by itself, handing that many owned rows to each neighbour
    bool masked = false;        // Dirichlet-mask grid: uniform chunks, every tile an ordinary tile
    bool multi = false;         // one of several passes in one launch (k_fused_multi): side sub-tiles of one height
};

struct FusedPlan {
    int T = 0, channels = 0;
    // the tiling, under FusedParams' names
    int st_lo = 0, st_hi = 0, rows_per_chunk = 0, first_rows = 0, last_rows = 0, n_strips = 0, n_chunks = 0;
    int nb_top = 0, nb_bot = 0, ns_left = 0, ns_right = 0;
    int side_rows = 0, side_subs = 1, side_rows_edge = 0;
    int first_edge = 0, last_edge = 0;
    int wide_y0 = 0, wide_y1 = 0, wide_h = 2, wide_nseg = 0, wide_stride = 1, wide_tiles = 0;
    unsigned long long edge_target = 0;
    // the launch shape
    int edge_chunks = 0, edge_strips = 0;   // chunk rows / strips whose tiles are border tiles
    long n_border = 0;                      // tiles of the border launch, per channel
    bool any_plain = false;                 // there are ordinary tiles
    bool edge = false;                      // the EDGE kernels: edge chunks first, in-launch signal
    bool wide = false;                      // the ordinary tiles run on wide strips
    int wx0 = 0, wx1 = 0, n_wide = 0;       // the columns of the wide interior and its strips
    WideBorder border;                      // what the segment planner was charged for the border launch
    unsigned grid_x = 0, grid_y = 0;        // ordinary launch (x z = channels), narrow strips
    unsigned bgrid_x = 0;                   // border launch (x 1 x channels)
    unsigned wgrid_x = 0;                   // wide launch (flat)
};

// ---- image edges ----------------------------------------------------------------------------------------------------
// Only IMAGE edges need the border arithmetic.  At the stale edge of a ghost zone the rows next to the edge are invalid
// by construction (validity recedes one row per half-sweep, they are neither stored nor used), so a tile there is an
// ordinary tile: the rows beyond the block read as 0.
inline bool fused_rows_at_top(const Geom &g, int ra, int T) { return g.y0 + ra - 2 * T <= 0; }
inline bool fused_rows_at_bottom(const Geom &g, int rb, int T) { return g.y0 + rb + 2 * T >= g.H - 1; }
// A chunk row at an image edge is cut short: 2T + 16 rows, enough for the chunk next to it to be clear of the edge (its
// halo starts below image row 0 / ends above image row H-1).
inline int fused_edge_short_rows(int T) { return 2 * T + 16; }

// Which tiles of a pass can touch a pixel with a missing neighbour: leading / trailing chunks by rows, leading /
// trailing strips by columns.  edge_rows > 0 (row block with neighbours, the pass whose result is exchanged): chunk 0 /
// the last chunk are cut to exactly the owned rows the upper / lower neighbour takes, so they finish — and are
// signalled — early (first_edge / last_edge).  Expects st_lo, st_hi, rows_per_chunk and n_strips in P.
inline void fused_tile_counts(const FusedPlanInput &in, int T, FusedPlan &P, int edge_rows)
{
    const Geom &geo = in.g;
    const int R = P.rows_per_chunk;
    const int rows = P.st_hi - P.st_lo;
    const int edge_short = fused_edge_short_rows(T);
    const bool at_top = fused_rows_at_top(geo, P.st_lo, T), at_bot = fused_rows_at_bottom(geo, P.st_hi, T);
    const bool cut = in.short_edges && rows > 2 * edge_short + R / 2 && R > edge_short;
    P.first_rows = (cut && at_top) ? edge_short : 0;
    P.last_rows = (cut && at_bot) ? edge_short : 0;
    P.first_edge = P.last_edge = 0;
    if (edge_rows > 0) {
        // rows from the first / last stored row that cover the neighbour's share of the owned rows
        int want_top = (in.stale_top && !at_top) ? geo.own_lo + std::min(edge_rows, in.send_up > 0 ? in.send_up : edge_rows) - P.st_lo : 0;
        int want_bot = (in.stale_bottom && !at_bot) ? P.st_hi - (geo.own_hi - std::min(edge_rows, in.send_down > 0 ? in.send_down : edge_rows)) : 0;
        want_top += want_top & 1;
        want_bot += want_bot & 1;
        const int others = P.first_rows + P.last_rows;
        if (want_top > 0 && want_bot > 0 && rows < want_top + want_bot + others + 2) want_top = want_bot = 0;   // too thin a block
        if (want_top > 0 && rows >= want_top + others + 2 && P.first_rows == 0) {
            P.first_rows = want_top;
            P.first_edge = 1;
        }
        if (want_bot > 0 && rows >= want_bot + P.first_rows + 2 && P.last_rows == 0) {
            P.last_rows = want_bot;
            P.last_edge = 1;
        }
    }
    const int mid = rows - P.first_rows - P.last_rows;
    if (P.first_edge || P.last_edge) {
        // the edge chunks take tile slots too: give the middle correspondingly fewer, taller chunks, so the
        // pass needs no more rounds on the chip's wave slots than it would without the hand-off (one
        // workgroup past a whole round costs a round).  (Round 3 tried the alternative — regular chunks of the usual
        // height plus short FOLLOW-UP chunks dispatched last, which take over the slots the edge tiles free after a
        // third of the pass: 0.760 ms per 32-iteration interval of a 2048-row block against 0.752 ms for this scheme and
        // 0.714 ms without the hand-off, profiles/r03_rank_block_edges.jsonl — two more chunk rows of halo cost what
        // the better packing saves.)
        const int n_whole = (rows + R - 1) / R;
        const int n_mid = std::max(1, n_whole - P.first_edge - P.last_edge);
        int r_mid = (mid + n_mid - 1) / n_mid;
        r_mid += r_mid & 1;
        P.rows_per_chunk = std::max(R, r_mid);
    }
    P.n_chunks = (mid + P.rows_per_chunk - 1) / P.rows_per_chunk + (P.first_rows > 0) + (P.last_rows > 0);
    auto top = [&](int c) { int ra, rb; fused_chunk_rows(P, c, ra, rb); return fused_rows_at_top(geo, ra, T); };
    auto bot = [&](int c) { int ra, rb; fused_chunk_rows(P, c, ra, rb); return fused_rows_at_bottom(geo, rb, T); };
    P.nb_top = 0;
    while (P.nb_top < P.n_chunks && top(P.nb_top)) ++P.nb_top;
    P.nb_bot = 0;
    while (P.nb_top + P.nb_bot < P.n_chunks && bot(P.n_chunks - 1 - P.nb_bot)) ++P.nb_bot;
    const int U = fused_useful_px(T);
    auto left = [&](int s) { return s * U - fused_halo_px(T) <= 0; };
    auto right = [&](int s) { return s * U - fused_halo_px(T) + 2 * kStripLanes >= geo.W - 1; };
    P.ns_left = 0;
    while (P.ns_left < P.n_strips && left(P.ns_left)) ++P.ns_left;
    P.ns_right = 0;
    while (P.ns_left + P.ns_right < P.n_strips && right(P.n_strips - 1 - P.ns_right)) ++P.ns_right;
    if (in.all_border) {                 // debug: every tile through the border launch
        P.nb_top = P.n_chunks;
        P.nb_bot = 0;
    }
}

// Side-strip tiles take ~2.5x the time per march step of an ordinary tile -> 2/5 of its march length.  The side strips
// of an EDGE pass's edge chunks are cut finer still (a sub-tile pays 4T rows of halo march whatever its height: 16 rows
// end at about half a pass), and side_subs covers the tallest of them; the passes of a multi-pass launch never signal and
// keep one height (edge_sub_tiles = false).
inline void fused_side_tiles(const FusedPlanInput &in, int T, FusedPlan &P, bool edge_sub_tiles)
{
    const int HS = 2 * T, R = P.rows_per_chunk;               // (possibly raised by fused_tile_counts for an edge pass)
    int sr = std::max(16, (R + 2 * HS) * 2 / 5 - 2 * HS);
    sr += sr & 1;
    if (in.side_rows_override > 0) sr = std::max(2, in.side_rows_override);
    P.side_rows = std::min(sr, R);
    P.side_subs = (R + P.side_rows - 1) / P.side_rows;
    P.side_rows_edge = edge_sub_tiles ? std::min(P.side_rows, 16) : P.side_rows;
    if (edge_sub_tiles && (P.first_edge || P.last_edge))
        P.side_subs = std::max(P.side_subs, (std::max(P.first_rows, P.last_rows) + P.side_rows_edge - 1) / P.side_rows_edge);
}

// A Dirichlet-mask grid: every tile an ordinary tile, uniform chunks (zero lies outside the block as it does outside
// the region).
inline void fused_uniform_tiling(FusedPlan &P)
{
    P.first_rows = P.last_rows = P.first_edge = P.last_edge = 0;
    P.n_chunks = (P.st_hi - P.st_lo + P.rows_per_chunk - 1) / P.rows_per_chunk;
    P.nb_top = P.nb_bot = P.ns_left = P.ns_right = 0;
    P.side_rows = P.side_rows_edge = P.rows_per_chunk;
    P.side_subs = 1;
}

// In-launch signal: every wave of an edge chunk (inner strips: one wave per strip in either kernel; edge strips: one
// wave per non-empty sub-tile) counts itself once per channel.
inline unsigned long long fused_edge_target(const FusedPlan &P)
{
    long waves_expected = 0;
    for (int c = 0; c < P.n_chunks; c += std::max(1, P.n_chunks - 1)) {      // chunk 0 and chunk n_chunks-1, once each
        if (!fused_is_edge_chunk(P, c)) continue;
        int ra, rb;
        fused_chunk_rows(P, c, ra, rb);
        const int subs = std::min(P.side_subs, (rb - ra + P.side_rows_edge - 1) / P.side_rows_edge);
        waves_expected += (P.n_strips - P.edge_strips) + (long)P.edge_strips * subs;
    }
    return (unsigned long long)waves_expected * P.channels;
}

// The ordinary tiles of an unchecked depth-8 pass run on wide strips (k_fused_sweep_wide): the columns [wx0, wx1) that
// the inner narrow strips would store, in the rows of the chunks between the border chunk rows.  The border tiles keep
// the narrow tiling, so ns_left / ns_right and the red-skip argument at fused_wave hold as they are.  The interior rows
// are one contiguous range, cut into segments sized to the device's wave slots instead of into the chunks
// (ccp_wide_plan.hpp); the launch is a flat list of tiles.
inline void fused_wide_interior(const FusedPlanInput &in, FusedPlan &P)
{
    const int T = P.T;
    int t;
    fused_chunk_rows(P, P.nb_top, P.wide_y0, t);
    fused_chunk_rows(P, P.n_chunks - P.nb_bot - 1, t, P.wide_y1);
    const int rows = P.wide_y1 - P.wide_y0;
    const long per_seg = (long)P.n_wide * P.channels;
    // what the border kernel has to march beside the wide tiles (ccp_wide_plan.hpp: the plan leaves it CUs)
    WideBorder &border = P.border;
    for (int e = 0; e < P.edge_chunks; ++e) {
        int ra, rb;
        fused_chunk_rows(P, e < P.nb_top ? e : P.n_chunks - P.edge_chunks + e, ra, rb);
        border.steps += (long)(rb - ra + 4 * T) * (P.n_strips - P.edge_strips);
        border.longest = std::max(border.longest, rb - ra + 4 * T);
    }
    if (P.edge_strips > 0) {
        border.steps += (long)P.n_chunks * P.edge_strips * P.side_subs * (P.side_rows + 4 * T);
        border.longest = std::max(border.longest, P.side_rows + 4 * T);
    }
    border.steps *= P.channels;
    const int slots = kWideWaves * in.cus;
    const WidePlan plan = in.wide_segments == 0 ? wide_plan_height(rows, P.rows_per_chunk)
                          : in.wide_segments > 0 ? wide_plan_count(rows, in.wide_segments)
                                                 : wide_plan(P.wide_y0, P.wide_y1, per_seg, slots, T, border);
    P.wide_h = plan.h;
    P.wide_nseg = plan.n_seg;
    // (the A/B form pads every segment's strips to whole blocks: exactly the blocks of the per-chunk grid it stands for)
    P.wide_stride = in.wide_segments == 0 ? (P.n_wide + kWideWaves - 1) / kWideWaves * kWideWaves : P.n_wide;
    P.wide_tiles = P.wide_stride * plan.n_seg * P.channels;
}

// The whole plan of one pass.
inline FusedPlan fused_plan(const FusedPlanInput &in, const FusedPassKind &k)
{
    FusedPlan P;
    const int T = k.T;
    P.T = T;
    P.channels = in.channels;
    P.st_lo = k.st_lo;
    P.st_hi = k.st_hi;
    P.rows_per_chunk = in.rows_per_chunk;
    P.n_strips = fused_n_strips(in.g.W, T);
    if (k.masked) {
        fused_uniform_tiling(P);
        P.any_plain = true;
    } else {
        fused_tile_counts(in, T, P, k.multi ? 0 : k.edge_rows);
        fused_side_tiles(in, T, P, !k.multi);
        P.edge_chunks = std::min(P.nb_top + P.nb_bot, P.n_chunks);
        P.edge_strips = std::min(P.ns_left + P.ns_right, P.n_strips);
        P.n_border = (long)P.edge_chunks * (P.n_strips - P.edge_strips) + (long)P.n_chunks * P.edge_strips * P.side_subs;
        P.any_plain = P.edge_chunks < P.n_chunks && P.edge_strips < P.n_strips;
        P.edge = !k.multi && k.edge_rows > 0 && (P.first_edge || P.last_edge);
        if (P.edge) P.edge_target = fused_edge_target(P);
        const int U = fused_useful_px(T);
        P.wx0 = P.ns_left * U;
        P.wx1 = (P.n_strips - P.ns_right) * U;
        P.n_wide = (T == kWideT && P.any_plain) ? (P.wx1 - P.wx0 + wide_useful_px(T) - 1) / wide_useful_px(T) : 0;
        // (a row stride the wide march cannot step by — wide_rows_stride_ok, an image millions of pixels wide — keeps the
        // 128-px strips and their descriptor per row)
        P.wide = !k.multi && T == kWideT && in.wide && k.l1 == 0 && !P.edge && P.any_plain && P.n_wide > 0 &&
                 wide_rows_stride_ok(in.g.pitch * 16L);
        if (P.wide) fused_wide_interior(in, P);
    }
    P.grid_x = (unsigned)((P.n_strips + kTileWaves - 1) / kTileWaves);
    P.grid_y = (unsigned)P.n_chunks;
    P.bgrid_x = (unsigned)((P.n_border + kTileWaves - 1) / kTileWaves);
    P.wgrid_x = (unsigned)((P.wide_tiles + kWideWaves - 1) / kWideWaves);
    return P;
}

// ---- ghost rows -----------------------------------------------------------------------------------------------------
// The local rows [lo, hi) a pass may store once `half_sweeps` half-sweeps have run since the last halo refresh, its own
// included: everything on a side that is the image border, and on a stale side one row fewer per half-sweep, down to the
// owned rows.  Pass k (from 0) of a run of depth-T passes that starts `since` half-sweeps after the refresh stores
// fused_stored_rows(in, since + 2 T (k + 1), ...).
inline void fused_stored_rows(const FusedPlanInput &in, int half_sweeps, int &lo, int &hi)
{
    lo = in.stale_top ? std::min(half_sweeps, in.ghost_top) : 0;
    hi = in.g.local_rows - (in.stale_bottom ? std::min(half_sweeps, in.ghost_bottom) : 0);
}
// Ghosts exhausted: that many half-sweeps need a refresh first.
inline bool fused_ghosts_exhausted(const FusedPlanInput &in, int half_sweeps)
{
    return (in.stale_top || in.stale_bottom) && half_sweeps > in.ghost;
}

// ---- a run of passes ------------------------------------------------------------------------------------------------
struct FusedPassSplit {
    std::vector<int> depths;    // the passes, deepest first; empty: no split exists
    int in_place = 0;           // iterations left to the in-place half-sweep kernels, after the passes
    bool free_parity = false;   // an odd number of passes: the result lands in the partner buffer
};

inline double fused_default_cost(int T) { return 1.0 + 0.01 * T; }   // "fewer, deeper launches are cheaper"

// Split `iterations` into an EVEN number of passes of depth <= tmax with the least total cost (cost[T], T = 1..tmax), so
// that the result lands back in the buffer it started in; an odd number where the caller allows it and it is cheaper.
// f[i][p]: best cost for i iterations with pass-count parity p.  Depth-1 passes only (tmax = 1) cannot cover an odd count
// in an even number of launches: the odd iteration is left to the in-place kernels.
inline FusedPassSplit fused_pass_split(int iterations, int tmax, const double *cost, bool free_parity_allowed)
{
    FusedPassSplit out;
    if (tmax == 1 && (iterations & 1)) {
        out.in_place = 1;
        iterations -= 1;
    }
    const double inf = 1e300;
    std::vector<double> f((size_t)(iterations + 1) * 2, inf);
    std::vector<int> step((size_t)(iterations + 1) * 2, 0);
    f[0] = 0.0;
    for (int i = 1; i <= iterations; ++i)
        for (int p = 0; p < 2; ++p)
            for (int T = 1; T <= tmax && T <= i; ++T) {
                const double c = f[(size_t)(i - T) * 2 + (p ^ 1)] + cost[T];
                if (c < f[(size_t)i * 2 + p]) {
                    f[(size_t)i * 2 + p] = c;
                    step[(size_t)i * 2 + p] = T;
                }
            }
    out.free_parity = free_parity_allowed && f[(size_t)iterations * 2 + 1] < f[(size_t)iterations * 2];
    for (int i = iterations, p = out.free_parity ? 1 : 0; i > 0;) {
        const int T = step[(size_t)i * 2 + p];
        if (T == 0) {
            out.depths.clear();
            return out;
        }
        out.depths.push_back(T);
        i -= T;
        p ^= 1;
    }
    std::sort(out.depths.begin(), out.depths.end(), std::greater<int>());
    return out;
}

// Pass k of n may leave out its red half (fused_wave says when that is safe) only when the pass after it in the same run
// is unchecked: the last pass stores both halves (whatever reads x after the call sees a whole buffer), and so does the
// pass before a checked one (l1_last: it reads the red of its input).
inline bool fused_stores_red(size_t k, size_t n, bool l1_last, bool red_store_all)
{
    return red_store_all || k + 1 >= n || (l1_last && k + 2 == n);
}

// ---- ccp_grid_tune --------------------------------------------------------------------------------------------------
// Chunk heights to time at depth T on a handle's local rows: fixed ones, plus those that fill `slots` resident
// workgroups in exactly 1..4 rounds — a short row block has few tiles, and one tile past a whole round costs a round.
// Chunk rows at an image edge are short ones of their own (fused_tile_counts).
inline std::vector<int> fused_tune_chunk_rows(const Geom &g, int channels, int T, long slots)
{
    std::vector<int> out = {32, 48, 64, 80, 96, 112, 128, 160, 192, 256};
    const int rows = g.local_rows;
    const long blocks_x = (fused_n_strips(g.W, T) + kTileWaves - 1) / kTileWaves;
    const int n_short = (int)fused_rows_at_top(g, 0, T) + (int)fused_rows_at_bottom(g, rows, T);
    const int short_rows = n_short * fused_edge_short_rows(T);
    for (int rounds = 1; rounds <= 4; ++rounds) {
        const long chunks = rounds * slots / (blocks_x * channels) - n_short;
        if (chunks < 1 || rows <= short_rows) continue;
        int R = (int)((rows - short_rows + chunks - 1) / chunks);
        R += R & 1;
        if (R >= 16 && R <= 1024 && std::find(out.begin(), out.end(), R) == out.end()) out.push_back(R);
    }
    return out;
}

}  // namespace ccp
