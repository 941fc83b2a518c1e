// ccp_wide_plan.hpp — how the interior rows of a wide depth-8 pass (ccp_grid_fused_wide.hpp) are cut into row
// segments, and how a tile reaches its rows (the rows of one ring turn, at the end).  Host-only arithmetic, no HIP:
// tests/cpp/wide_plan_check.cpp and tests/cpp/wide_rows_check.cpp include this header alone.
//
// One wave of k_fused_sweep_wide marches one (wide strip, row segment) tile, and its 40 KB ring of b/4 rows leaves room
// for one wave per SIMD: the device runs `slots` = 4 x CUs tiles at a time.  A tile of h stored rows marches h + 4T
// rows (2T rows of halo either side), rounded up to whole turns of the ring.  Without border tiles the plan is the
// segment count whose
//     rounds x march steps = ceil(strips x channels x n_seg / slots) x round_up(h + 4T, kWideRing)
// is smallest: as few rounds as possible on the wave slots, and in them segments as short as the slots allow.
//
// The border tiles of the pass run in another kernel (k_fused_border) beside the wide one, and a wide block fills its CU
// (all of its LDS, more than half of every SIMD's registers): a border block runs only on a CU that holds no wide block.
// Measured (NOTES R12.1): with every CU taken the border kernel starts when the wide waves end, and the pass is the sum
// of the two; with too few CUs left free it does not finish beside them either.  So a plan also pays the border
// kernel's tail — its longest wave, whose march steps take kWideBorderSlow x as long — unless it is hidden: one round,
// and the CUs it leaves free work off the border waves' march steps (kWideBorderPerCu of them per CU and wide march
// step: 8 waves at 1 / kWideBorderSlow of the rate, packed to about 0.6) within the wide march.
#pragma once

#if defined(__HIPCC__)
#define CCP_WIDE_PLAN_FN __host__ __device__ inline
#else
#define CCP_WIDE_PLAN_FN inline
#endif

namespace ccp {

constexpr int kWideRing = 20;       // b/4 rows per wave in LDS (ccp_grid_fused_wide.hpp); the march runs whole turns of it
constexpr int kWideMinSegRows = 64; // shortest planned segment: 4 x the 2T = 16 halo rows, i.e. at most 1.5x redundant rows

struct WidePlan {
    int n_seg;   // segments; segment s holds rows [y0 + s h, min(y0 + (s + 1) h, y1))
    int h;       // rows per segment (the last one may be shorter)
};

inline int wide_march_steps(int h, int T) { return (h + 4 * T + kWideRing - 1) / kWideRing * kWideRing; }

struct WideBorder {
    long steps = 0;    // march steps of all border waves of the pass (rows + 4T each), every channel
    int longest = 0;   // march steps of the longest border wave
};
constexpr int kWideBorderPerCu = 2;                  // border march steps a free CU works off per wide march step
constexpr int kWideBorderSlowNum = 5, kWideBorderSlowDen = 2;   // a border wave's march step against a wide wave's

inline long wide_plan_cost(long tiles_per_segment, int n_seg, int h, int slots, int T, const WideBorder &border = WideBorder())
{
    const long tiles = tiles_per_segment * n_seg;
    const long rounds = (tiles + slots - 1) / slots;
    const long march = wide_march_steps(h, T);
    const long free_cus = slots / 4 - (tiles + 3) / 4;            // CUs without a wide block (one round)
    const bool hidden = border.steps == 0 || (rounds == 1 && kWideBorderPerCu * free_cus * march >= border.steps);
    return rounds * march + (hidden ? 0 : (long)border.longest * kWideBorderSlowNum / kWideBorderSlowDen);
}

// segments of a given height (h = R: the interior chunks of the narrow tiling)
inline WidePlan wide_plan_height(int rows, int h)
{
    if (h < 1) h = 1;
    return WidePlan{rows > 0 ? (rows + h - 1) / h : 0, h};
}

// n segments of one even height (fewer when the rounding of h leaves the last ones empty)
inline WidePlan wide_plan_count(int rows, int n)
{
    if (rows <= 0) return WidePlan{0, 2};
    if (n < 1) n = 1;
    int h = (rows + n - 1) / n;
    h += h & 1;
    return wide_plan_height(rows, h);
}

// The plan for interior rows [y0, y1), tiles_per_segment = wide strips x channels, slots = 4 x CUs, depth T.
inline WidePlan wide_plan(int y0, int y1, long tiles_per_segment, int slots, int T, const WideBorder &border = WideBorder())
{
    const int rows = y1 - y0;
    WidePlan best = wide_plan_count(rows, 1);
    if (rows <= 0 || tiles_per_segment <= 0 || slots <= 0) return best;
    long best_cost = wide_plan_cost(tiles_per_segment, best.n_seg, best.h, slots, T, border);
    for (int n = 2; n <= rows / kWideMinSegRows; ++n) {
        const WidePlan p = wide_plan_count(rows, n);
        if (p.n_seg != n || p.h < kWideMinSegRows) continue;     // (the same plan as a smaller n, or too short)
        const long cost = wide_plan_cost(tiles_per_segment, p.n_seg, p.h, slots, T, border);
        if (cost < best_cost) {                                  // ties go to fewer segments
            best = p;
            best_cost = cost;
        }
    }
    return best;
}

CCP_WIDE_PLAN_FN void wide_segment_rows(int y0, int y1, int h, int s, int &ra, int &rb)
{
    ra = y0 + s * h;
    rb = ra + h < y1 ? ra + h : y1;
}

// ---- the rows of one ring turn --------------------------------------------------------------------------------------
// A turn of the march (kWideRing steps, fully unrolled) touches one WINDOW of kWideRing consecutive rows per plane:
// it loads rows [fb + 2G, fb + 2G + kWideRing) of x and b and stores rows [fb - 2T, fb - 2T + kWideRing) of x, fb the
// newest row of its first step.  One buffer descriptor per plane and turn covers the window: its base is the window's
// first row w0 (never dereferenced where that row does not exist), and its num_records ends at the last row that exists.
// The window's k-th row (k a compile-time constant of the unrolled step) is reached by the byte offset k x stride; a row
// before the first existing one gets kWideRowOut instead, which no descriptor reaches.  So the range check alone selects
// exactly the rows of [lo, hi), as one descriptor per row did.
//
// A lane adds its own offset inside the row (< stride) or kLaneOut = 2^31 (ccp_grid_fused.hpp).  With
// (kWideRing + 4) x stride <= 2^30 (wide_rows_stride_ok) every sum stays below 2^32 and every num_records at or below
// kWideRowOut: nothing wraps, whatever the segment height, because the offsets restart from 0 every turn.
struct WideMarch {
    int m0, m1;    // rows the tile loads: its rows and 2T rows of halo either side, clipped to the rows of the block
    int base;      // newest row of the first step: m0, or m0 - 1 where that is the even image row (it does not exist then)
    int f_end;     // newest row of the step that stores row rb - 1; turns begin at base, base + kWideRing, ... <= f_end
};
// the march of a tile that stores rows [ra, rb) of a block of local_rows rows whose row 0 is image row y0, depth T
CCP_WIDE_PLAN_FN WideMarch wide_march(int ra, int rb, int local_rows, int y0, int T)
{
    WideMarch m;
    m.m0 = ra - 2 * T > 0 ? ra - 2 * T : 0;
    m.m1 = rb + 2 * T < local_rows ? rb + 2 * T : local_rows;
    m.base = m.m0 - ((y0 + m.m0) & 1);
    m.f_end = rb - 1 + 2 * T;
    return m;
}
constexpr int kWideLoadAhead = 4;               // a turn loads the rows [fb + 4, fb + 4 + kWideRing): two trips of G = 2 ahead

constexpr unsigned kWideRowOut = 0x40000000u;
constexpr int kWideRowSpan = kWideRing + 4;     // row strides the guard allows for: the window and the rows in flight around it

CCP_WIDE_PLAN_FN bool wide_rows_stride_ok(long stride_bytes)
{
    return stride_bytes >= 0 && stride_bytes <= (long)(kWideRowOut / kWideRowSpan);
}

struct WideTurnRows {
    int first;          // row at the descriptor's base: the window's first row
    int skip;           // rows of the window before the first one that exists: they take kWideRowOut
    unsigned records;   // bytes from the base to the end of the last row of the window that exists (0: none)
};

// window [w0, w0 + kWideRing), existing rows [lo, hi), stride in bytes (wide_rows_stride_ok)
CCP_WIDE_PLAN_FN WideTurnRows wide_turn_rows(int w0, int lo, int hi, unsigned stride)
{
    const int below = lo - w0, upto = hi - w0;
    WideTurnRows r;
    r.first = w0;
    r.skip = below < 0 ? 0 : below > kWideRing ? kWideRing : below;
    r.records = (unsigned)(upto < 0 ? 0 : upto > kWideRing ? kWideRing : upto) * stride;
    return r;
}

// byte offset of the window's k-th row from the descriptor's base
CCP_WIDE_PLAN_FN unsigned wide_row_offset(int k, int skip, unsigned stride)
{
    return k >= skip ? (unsigned)k * stride : kWideRowOut;
}

}  // namespace ccp
