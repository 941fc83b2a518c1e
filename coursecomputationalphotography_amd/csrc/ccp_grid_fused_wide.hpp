// ccp_grid_fused_wide.hpp — the depth-8 ordinary tiles of an unchecked pass on WIDE strips (k_fused_sweep_wide).
//
// Same schedule and arithmetic as fused_wave's kStepFast body (ccp_grid_fused.hpp); what differs is the geometry:
//   * lane i holds half-columns j0 + 2i and j0 + 2i + 1 of both colours (pixels A and B of the lane), so a wave covers
//     256 pixel columns and stores 256 - 4T of them (224 at T = 8: 1.14x redundant work against 1.33x on 128-px strips);
//     the two same-colour values are adjacent in the de-interleaved row, so every x load and store is one dwordx4 per
//     colour per row, and a colour's two updates per row need ONE lane shift (the other neighbour is in the lane);
//   * x stays in the register window (2T+3 rows x 8 VGPRs); b/4 does not: a landed b row is scaled by 1/4 once and
//     written to a ring of kWideRing rows in the wave's own part of LDS, where every update reads it (ds_read_b128).
//     The ring is indexed by row, so b is never shifted.  LDS instructions of one wave complete in order: no barrier,
//     no wait on another wave — one wavefront is still one worker;
//   * the ring's slot of a row is (row - base) mod kWideRing, a compile-time constant in every unrolled step because
//     the trip loop is unrolled over one whole turn of the ring (kWideRing / G trips);
//   * for the same reason a turn's rows are compile-time multiples of the row stride away from the turn's first row:
//     the wave builds its buffer descriptors once per turn and plane, not once per row (WideTurn below).  It runs alone
//     on its SIMD, where every scalar instruction of a descriptor per row was issue time nothing else filled.
// It runs only the interior: the columns [wx0, wx1) that the narrow ordinary strips would store (the narrow side
// strips stay border tiles in k_fused_border) and the rows between the top and bottom border chunks.  Those rows are one
// contiguous range, and nothing here needs the chunk height: the host cuts them into row SEGMENTS sized to the device's
// wave slots (ccp_wide_plan.hpp), and the launch is a flat list of (channel, segment, strip) tiles.  Every pixel
// column an interior wide strip stores or depends on (2T columns either side) lies in [1, W-2], so the plain stencil
// is exact wherever it matters; pixels further out are halo, computed with whatever was loaded and never stored.
#pragma once

#include "ccp_grid_fused.hpp"
#include "ccp_wide_plan.hpp"                  // kWideRing = 20 b/4 rows per wave in LDS: 2 KB each, 40 KB per wave, 160 KB per block

namespace ccp {

// kWideT, kWideWaves and wide_useful_px: ccp_fused_plan.hpp

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));   // the lane's pixels A and B of one colour

__device__ __forceinline__ d2 buf_load2(__amdgpu_buffer_rsrc_t rs, unsigned voff)
{
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
}
__device__ __forceinline__ void buf_store2(d2 v, __amdgpu_buffer_rsrc_t rs, unsigned voff)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (int)voff, 0, 0);
}

struct WideCtx {
    const double *__restrict__ xin;
    double *__restrict__ xout;
    const double *__restrict__ bb;
    unsigned ld_r, ld_k;   // byte offset of the lane's red / black pair inside a row, kLaneOut if its first half-column does not exist
    unsigned st_r, st_k;   // the same for stores: kLaneOut unless the strip stores both half-columns of the lane
    int ra, rb;            // rows to finalise and store
    int m0, m1;            // rows loaded
    d2 *ring;              // this lane's pair in slot 0, red half: ring[slot * 2 * kWave + c * kWave]
};

// row q: x red, x black, b red, b black (pairs); rows outside [m0, m1) read 0.  One descriptor per row (row_rsrc): the
// four rows the march starts with, before its first turn.
__device__ __forceinline__ void wide_load_row(const WideCtx &cx, const Geom &g, int q, d2 (&dst)[4])
{
    const bool exists = q >= cx.m0 && q < cx.m1;
    const __amdgpu_buffer_rsrc_t rx = row_rsrc(cx.xin, g, q, exists), rbb = row_rsrc(cx.bb, g, q, exists);
    dst[0] = buf_load2(rx, cx.ld_r);
    dst[1] = buf_load2(rx, cx.ld_k);
    dst[2] = buf_load2(rbb, cx.ld_r);
    dst[3] = buf_load2(rbb, cx.ld_k);
}

// The rows of one ring turn (ccp_wide_plan.hpp, wide_turn_rows): one descriptor per plane for the whole turn, rebuilt
// between turns from wave-uniform values, instead of one per row.  A row of the turn is a compile-time number of row
// strides from the descriptor's base, added to the lane's offset by one v_add_u32.
struct WideTurn {
    __amdgpu_buffer_rsrc_t rx, rbb, ro;   // x in and b over the rows the turn loads, x out over the rows it stores
    unsigned stride;                      // bytes per row (both colours)
    int st_skip;                          // rows of the store window before ra
};

// descriptor of `records` bytes at row `row` of `plane`; the inputs go through readfirstlane, so that the compiler
// knows the descriptor to be wave-uniform and puts no waterfall loop around the memory instructions that use it
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wide_window_rsrc(const double *plane, const Geom &g, int row, unsigned records)
{
    const unsigned long long a = (unsigned long long)(plane + (long)row * 2 * g.pitch);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    const int n = __builtin_amdgcn_readfirstlane((int)records);
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, n, 0x00020000);
}

// the turn whose first step has newest row fb: it loads rows [fb + 2G, fb + 2G + kWideRing) and stores rows
// [fb - 2T, fb - 2T + kWideRing).  A loaded row is never before m0 (fb >= base >= m0 - 1), so only the stores skip rows.
template <int T>
__device__ __forceinline__ WideTurn wide_turn_begin(const WideCtx &cx, const Geom &g, int fb)
{
    constexpr int G = 2;
    static_assert(kWideLoadAhead == 2 * G, "ccp_wide_plan.hpp describes this march");
    WideTurn t;
    t.stride = (unsigned)g.pitch * 16u;
    // The stride is the same in every turn, and the compiler, seeing that, would form lane offset + k x stride for all
    // k once, ahead of the march, in 40 registers the window needs.  Taken through an empty asm it is a new value per
    // turn: each sum is formed where it is used and dies with its memory instruction.
    asm volatile("" : "+s"(t.stride));
#if defined(CCP_WIDE_PROBE_DESC)
    // timing-only experiment (results are wrong): every row of the turn is the turn's first row, clamped into the
    // rows that exist, and exists; the per-row scalar work is gone from the instruction stream
    const int ql = min(max(fb + 2 * G, cx.m0), cx.m1 - 1), qs = min(max(fb - 2 * T, cx.ra), cx.rb - 1);
    t.rx = wide_window_rsrc(cx.xin, g, ql, t.stride);
    t.rbb = wide_window_rsrc(cx.bb, g, ql, t.stride);
    t.ro = wide_window_rsrc(cx.xout, g, qs, t.stride);
    t.st_skip = 0;
#else
    const WideTurnRows ld = wide_turn_rows(fb + 2 * G, cx.m0, cx.m1, t.stride);
    const WideTurnRows st = wide_turn_rows(fb - 2 * T, cx.ra, cx.rb, t.stride);
    t.rx = wide_window_rsrc(cx.xin, g, ld.first, ld.records);
    t.rbb = wide_window_rsrc(cx.bb, g, ld.first, ld.records);
    t.ro = wide_window_rsrc(cx.xout, g, st.first, st.records);
    t.st_skip = st.skip;
#endif
    return t;
}

// byte offset of the turn's k-th loaded / stored row from its descriptor's base
__device__ __forceinline__ unsigned wide_ld_row(const WideTurn &t, int k)
{
#if defined(CCP_WIDE_PROBE_DESC)
    return 0u;
#else
    return wide_row_offset(k, 0, t.stride);      // (no loaded row of a turn is before m0: wide_turn_begin)
#endif
}
__device__ __forceinline__ unsigned wide_st_row(const WideTurn &t, int k)
{
#if defined(CCP_WIDE_PROBE_DESC)
    return 0u;
#else
    return wide_row_offset(k, t.st_skip, t.stride);
#endif
}

// the k-th row of the turn's load window: x red, x black, b red, b black (pairs); rows from m1 on read 0
__device__ __forceinline__ void wide_load_turn_row(const WideCtx &cx, const WideTurn &t, int k, d2 (&dst)[4])
{
    const unsigned row = wide_ld_row(t, k);
    dst[0] = buf_load2(t.rx, cx.ld_r + row);
    dst[1] = buf_load2(t.rx, cx.ld_k + row);
    dst[2] = buf_load2(t.rbb, cx.ld_r + row);
    dst[3] = buf_load2(t.rbb, cx.ld_k + row);
}

__host__ __device__ constexpr int wide_slot(int k) { return ((k % kWideRing) + kWideRing) % kWideRing; }

// One march step (fused_step's kStepFast): newest row f = fb + i, half-sweep h on row f - h, then the store of row
// f - 2T, the (PH + i)-th row of the turn's store window.  PH: ring slot of row fb.
template <int T, bool STORE_RED, int NT, int PH>
__device__ __forceinline__ void wide_step(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const WideTurn &t, int i)
{
    using Win = FusedWindow<T, 2>;
    constexpr int HS = Win::HS;
#pragma unroll
    for (int h = 1; h <= HS; ++h) {
        const int sr = Win::slot(i, h), su = Win::slot(i, h + 1), sd = Win::slot(i, h - 1);
        const int c = (h - 1) & 1;                       // 0 = red, 1 = black
        const int p = ((i - h + 2 * HS + 2) + c) & 1;    // pixel A is column 2 jA + p, pixel B 2 jA + 2 + p
        const d2 up = c ? wr[su] : wk[su];
        const d2 dn = c ? wr[sd] : wk[sd];
        const d2 o = c ? wr[sr] : wk[sr];                // the opposite colour in the same row
        double la, ra, lb, rb;
        if (p == 0) {                                    // A's left is the previous lane's B
            la = lane_prev(o.y); ra = o.x; lb = o.x; rb = o.y;
        } else {                                         // B's right is the next lane's A
            la = o.x; ra = o.y; lb = o.y; rb = lane_next(o.x);
        }
        const d2 bq = cx.ring[wide_slot(PH + i - h) * 2 * kWave + c * kWave];
        d2 nv;
        nv.x = __builtin_fma(((up.x + la) + ra) + dn.x, 0.25, bq.x);
        nv.y = __builtin_fma(((up.y + lb) + rb) + dn.y, 0.25, bq.y);
        if (c) wk[sr] = nv; else wr[sr] = nv;
    }
    {
        const int sr = Win::slot(i, HS);
        const unsigned row = wide_st_row(t, PH + i);
        if constexpr (STORE_RED) buf_store2(wr[sr], t.ro, cx.st_r + row);
        buf_store2(wk[sr], t.ro, cx.st_k + row);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// a landed row: x into window slot s0, b/4 into ring slot `slot`
template <int NT>
__device__ __forceinline__ void wide_place(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, int s0, int slot, const d2 (&row)[4])
{
    wr[s0] = row[0];
    wk[s0] = row[1];
    cx.ring[slot * 2 * kWave] = row[2] * 0.25;
    cx.ring[slot * 2 * kWave + kWave] = row[3] * 0.25;
}

// One trip (G = 2 steps) of the two-landing-pair march (fused_wave, kFusedLand = 2): issue the loads of the rows two
// trips ahead into LANDING, run the steps, shift the window, move the rows of ARRIVED in.  PH: ring slot of row fb,
// and the place of the trip's rows in the turn's load and store windows.
template <int T, bool STORE_RED, int NT, int PH>
__device__ __forceinline__ void wide_trip(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const WideTurn &t,
                                          d2 (&landing)[2][4], const d2 (&arrived)[2][4])
{
    constexpr int G = 2;
    using Win = FusedWindow<T, G>;
#pragma unroll
    for (int i = 0; i < G; ++i) wide_load_turn_row(cx, t, PH + i, landing[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i == 0) wide_step<T, STORE_RED, NT, PH>(wr, wk, cx, t, 0);
        else wide_step<T, STORE_RED, NT, PH>(wr, wk, cx, t, 1);
    }
#pragma unroll
    for (int s = 0; s + G < NT; ++s) {
        wr[s] = wr[s + G];
        wk[s] = wk[s + G];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) wide_place(wr, wk, cx, Win::slot(i, 0), wide_slot(PH + G + i), arrived[i]);
}

// One turn of the ring: kWideRing / G trips starting at ring slot PH (trip k: landing pair k & 1).  No exit between
// the trips of a turn: with one, the compiler sinks each trip's loads below the test into the next trip, where they
// are used, and the wave waits for every row it loads.  Trips past the end of the march store nothing (the rows are
// outside [ra, rb)) and load zeros (outside [m0, m1)).
template <int T, bool STORE_RED, int NT, int PH>
__device__ __forceinline__ void wide_turn(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const WideTurn &t,
                                          d2 (&la)[2][4], d2 (&lb)[2][4])
{
    if constexpr (PH < kWideRing) {
        if constexpr ((PH / 2) % 2 == 0) wide_trip<T, STORE_RED, NT, PH>(wr, wk, cx, t, la, lb);
        else wide_trip<T, STORE_RED, NT, PH>(wr, wk, cx, t, lb, la);
        wide_turn<T, STORE_RED, NT, PH + 2>(wr, wk, cx, t, la, lb);
    }
}

// One wave: wide strip sw (stored columns [wx0 + sw U, ...) clipped to wx1), rows [ra, rb).
template <int T, bool STORE_RED>
__device__ __forceinline__ void fused_wave_wide(const double *__restrict__ xin, double *__restrict__ xout,
                                                const double *__restrict__ bb, const Geom &g, int wx0, int wx1, int sw,
                                                int ra, int rb, d2 *ring)
{
    static_assert(T % 2 == 0, "the lane pairs line up with the stored columns only for an even depth");
    constexpr int G = 2;
    static_assert(kWideRing % (2 * G) == 0 && kWideRing >= 2 * T + 2 * G, "the ring holds the rows a trip reads and the rows it lands");
    using Win = FusedWindow<T, G>;
    constexpr int HS = Win::HS, NT = Win::NT;
    const int lane = (int)(threadIdx.x & (kWave - 1));
    WideCtx cx;
    cx.xin = xin; cx.xout = xout; cx.bb = bb;
    cx.ring = ring + lane;
    const int x0 = wx0 + sw * wide_useful_px(T);
    const int x1 = min(x0 + wide_useful_px(T), wx1);        // stored pixel columns [x0, x1), both even
    const int ja = (x0 - fused_halo_px(T)) / 2 + 2 * lane;   // the lane's first half-column
    const bool col_ok = ja >= 0 && ja < g.pitch;
    const bool col_store = col_ok && 2 * ja >= x0 && 2 * ja + 3 < x1;
    cx.ld_r = col_ok ? (unsigned)ja * 8u : kLaneOut;
    cx.ld_k = col_ok ? (unsigned)(g.pitch + ja) * 8u : kLaneOut;
    cx.st_r = (STORE_RED && col_store) ? cx.ld_r : kLaneOut;
    cx.st_k = col_store ? cx.ld_k : kLaneOut;
    cx.ra = ra; cx.rb = rb;
    const WideMarch mar = wide_march(ra, rb, g.local_rows, g.y0, T);
    cx.m0 = mar.m0;
    cx.m1 = mar.m1;
    const int base = mar.base;                               // even image row: compile-time colour parity per step
    const int f_end = mar.f_end;

    d2 wr[NT], wk[NT];
    d2 la[G][4], lb[G][4];
#pragma unroll
    for (int s = 0; s < NT; ++s) wr[s] = wk[s] = d2{0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kWideRing; ++s) {                   // rows before `base` (halo beyond the halo) read b = 0
        cx.ring[s * 2 * kWave] = d2{0.0, 0.0};
        cx.ring[s * 2 * kWave + kWave] = d2{0.0, 0.0};
    }
#pragma unroll
    for (int i = 0; i < G; ++i) wide_load_row(cx, g, base + i, la[i]);
#pragma unroll
    for (int i = 0; i < G; ++i) wide_load_row(cx, g, base + G + i, lb[i]);
#pragma unroll
    for (int i = 0; i < G; ++i) wide_place(wr, wk, cx, Win::slot(i, 0), i, la[i]);
    for (int fb = base; fb <= f_end; fb += kWideRing) {
        const WideTurn t = wide_turn_begin<T>(cx, g, fb);
        wide_turn<T, STORE_RED, NT, 0>(wr, wk, cx, t, la, lb);
    }
}

// grid = ceil(wide_tiles / 4) blocks; block = 4 waves = 4 consecutive tiles.  Tile t = (channel * wide_nseg + segment) *
// wide_stride + strip, strip fastest (wide_stride = n_wide, but for the A/B form of the old per-chunk blocks): the waves
// of a block are adjacent wide strips of one segment (they share their halo columns in L1 / L2) and every block but the
// last is full.  The tiles of a pass are independent (xin -> xout).
template <int T, bool STORE_RED>
__global__ void __launch_bounds__(kBlock, 2)
k_fused_sweep_wide(FusedParams P, int wx0, int wx1, int n_wide)
{
    __shared__ d2 ring[kWideWaves][kWideRing * 2 * kWave];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    unsigned bx, by, bz;
    fused_tile_coords(P, bx, by, bz);
    const int tile = (int)bx * kWideWaves + wave;
    if (tile >= P.wide_tiles) return;
    const int row = tile / P.wide_stride;         // channel * wide_nseg + segment
    const int sw = tile - row * P.wide_stride;
    if (sw >= n_wide) return;                     // (CCP_GS_WIDE_SEGMENTS=0 pads a row to whole blocks)
    const int ch = row / P.wide_nseg;
    const int seg = row - ch * P.wide_nseg;
    int ra, rb;
    wide_segment_rows(P.wide_y0, P.wide_y1, P.wide_h, seg, ra, rb);
    const bool run = (P.active == nullptr) || (P.active[ch] != 0);
    if (run && ra < rb) {
        const Geom &g = P.g;
        const long off = (long)ch * g.ch_stride;
        unsigned long long t0 = 0;
        fused_trace_begin(P, t0);
        fused_wave_wide<T, STORE_RED>(P.xin + off, P.xout + off, P.b + off, g, wx0, wx1, sw, ra, rb, ring[wave]);
        fused_trace_end(P, t0, tile, seg, sw, ch, 3);      // slot = tile id, chunk field = segment
    }
}

}  // namespace ccp
