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
//     the trip loop is unrolled over one whole turn of the ring (kWideRing / G trips).
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

// row q: x red, x black, b red, b black (pairs); rows outside [m0, m1) read 0
__device__ __forceinline__ void wide_load_row(const WideCtx &cx, const Geom &g, int q, d2 (&dst)[4])
{
    const bool exists = q >= cx.m0 && q < cx.m1;
    const __amdgpu_buffer_rsrc_t rx = row_rsrc(cx.xin, g, q, exists), rbb = row_rsrc(cx.bb, g, q, exists);
    dst[0] = buf_load2(rx, cx.ld_r);
    dst[1] = buf_load2(rx, cx.ld_k);
    dst[2] = buf_load2(rbb, cx.ld_r);
    dst[3] = buf_load2(rbb, cx.ld_k);
}

__host__ __device__ constexpr int wide_slot(int k) { return ((k % kWideRing) + kWideRing) % kWideRing; }

// One march step (fused_step's kStepFast): newest row f = fb + i, half-sweep h on row f - h, then the store of row
// f - 2T.  PH: ring slot of row fb.
template <int T, bool STORE_RED, int NT, int PH>
__device__ __forceinline__ void wide_step(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const Geom &g, int f, int i)
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
        const int r = f - HS;
        const int sr = Win::slot(i, HS);
        const __amdgpu_buffer_rsrc_t ro = row_rsrc(cx.xout, g, r, r >= cx.ra && r < cx.rb);
        if constexpr (STORE_RED) buf_store2(wr[sr], ro, cx.st_r);
        buf_store2(wk[sr], ro, cx.st_k);
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
// trips ahead into LANDING, run the steps, shift the window, move the rows of ARRIVED in.  PH: ring slot of row fb.
template <int T, bool STORE_RED, int NT, int PH>
__device__ __forceinline__ void wide_trip(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const Geom &g, int fb,
                                          d2 (&landing)[2][4], const d2 (&arrived)[2][4])
{
    constexpr int G = 2;
    using Win = FusedWindow<T, G>;
#pragma unroll
    for (int i = 0; i < G; ++i) wide_load_row(cx, g, fb + 2 * G + i, landing[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i == 0) wide_step<T, STORE_RED, NT, PH>(wr, wk, cx, g, fb, 0);
        else wide_step<T, STORE_RED, NT, PH>(wr, wk, cx, g, fb + 1, 1);
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
__device__ __forceinline__ void wide_turn(d2 (&wr)[NT], d2 (&wk)[NT], const WideCtx &cx, const Geom &g, int fb,
                                          d2 (&la)[2][4], d2 (&lb)[2][4])
{
    if constexpr (PH < kWideRing) {
        if constexpr ((PH / 2) % 2 == 0) wide_trip<T, STORE_RED, NT, PH>(wr, wk, cx, g, fb, la, lb);
        else wide_trip<T, STORE_RED, NT, PH>(wr, wk, cx, g, fb, lb, la);
        wide_turn<T, STORE_RED, NT, PH + 2>(wr, wk, cx, g, fb + 2, la, lb);
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
    cx.m0 = max(ra - HS, 0);
    cx.m1 = min(rb + HS, g.local_rows);
    const int base = cx.m0 - ((g.y0 + cx.m0) & 1);          // even image row: compile-time colour parity per step
    const int f_end = rb - 1 + HS;

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
    for (int fb = base; fb <= f_end; fb += kWideRing) wide_turn<T, STORE_RED, NT, 0>(wr, wk, cx, g, fb, la, lb);
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
