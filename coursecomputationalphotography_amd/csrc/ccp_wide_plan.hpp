// ccp_wide_plan.hpp — how the interior rows of a wide depth-8 pass (ccp_grid_fused_wide.hpp) are cut into row
// segments.  Host-only arithmetic, no HIP: tests/cpp/wide_plan_check.cpp includes this header alone.
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

}  // namespace ccp
