// ccp_grid_blend.hpp — both ends of a region blend on a Dirichlet-mask grid (CCP_GRID_DIRICHLET_MASK):
// b (and optionally x) from host images in one pass, and the composite epilogue.  See include/ccp_gs.h
// (ccp_grid_assemble_region_rhs, ccp_grid_assemble_clone, ccp_grid_store_u8_composite).
//
// One thread per pixel of a local row; the channels are a loop inside the thread, so the mask and the
// neighbour rows' region bytes are read once per pixel whatever the channel count.  Images are read through
// accessors (ccp_grid_io.hpp) indexed by IMAGE row: the host entry points stage a row window of the canvas (the
// local rows plus one row above and one below where they exist), the _device twins read the caller's whole-canvas
// strided views and touch the same rows.  Region membership of a pixel comes from the split mask (`mask`, the
// layout of x) on local rows and from `edge` (2 x W bytes: image row y0-1, then image row y0+local_rows;
// zero where the row does not exist) one row beyond them.
#pragma once

#include "ccp_grid_io.hpp"
#include "ccp_grid_stencil.hpp"

#include <cstdint>

namespace ccp {

struct BlendMask {
    const unsigned char *__restrict__ mask;
    const unsigned char *__restrict__ edge;
    Geom g;
    // is local row ll (-1 .. local_rows), column xx (inside the canvas) a pixel of the region?
    __device__ __forceinline__ bool at(int ll, int xx) const
    {
        if (ll < 0) return edge[xx] != 0;
        if (ll >= g.local_rows) return edge[g.W + xx] != 0;
        return mask[row_off(g, ll, (xx + g.y0 + ll) & 1) + (xx >> 1)] != 0;
    }
};

// Field form (lab8's union region, hw8_pa.cc:749-810; lab8_workload.region_system's operation order): for a
// region pixel, in double with the float fields widened,
//     t = 0 - (gx + gy);  t += gx(x-1,y) if x >= 1;  t += gy(x,y-1) if y >= 1
//     o = 0;  o += N, S, W, E  (canvas value of a neighbour inside the canvas and outside the region, else 0)
//     b = t + o
// b = 0 outside the region.  INIT: x := canvas inside the region, 0 outside.
// grid = (ceil(W / kBlock), local_rows).
template <bool INIT, typename F, typename U>
__global__ void __launch_bounds__(kBlock)
k_blend_field_rhs(double *__restrict__ b, double *__restrict__ x, BlendMask r, F gx, F gy, U canvas, int C)
{
    const Geom &g = r.g;
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    const int l = blockIdx.y;
    if (xi >= g.W) return;
    const int y = g.y0 + l;
    const long at = row_off(g, l, (xi + y) & 1) + (xi >> 1);
    if (!r.mask[at]) {
        for (int ch = 0; ch < C; ++ch) {
            b[(long)ch * g.ch_stride + at] = 0.0;
            if (INIT) x[(long)ch * g.ch_stride + at] = 0.0;
        }
        return;
    }
    const bool oN = y >= 1 && !r.at(l - 1, xi);
    const bool oS = y + 1 < g.H && !r.at(l + 1, xi);
    const bool oW = xi >= 1 && !r.at(l, xi - 1);
    const bool oE = xi + 1 < g.W && !r.at(l, xi + 1);
    for (int ch = 0; ch < C; ++ch) {
        double t = 0.0 - ((double)gx(y, xi, ch) + (double)gy(y, xi, ch));
        if (xi >= 1) t += (double)gx(y, xi - 1, ch);
        if (y >= 1) t += (double)gy(y - 1, xi, ch);
        double o = 0.0;
        o += oN ? (double)canvas(y - 1, xi, ch) : 0.0;
        o += oS ? (double)canvas(y + 1, xi, ch) : 0.0;
        o += oW ? (double)canvas(y, xi - 1, ch) : 0.0;
        o += oE ? (double)canvas(y, xi + 1, ch) : 0.0;
        b[(long)ch * g.ch_stride + at] = t + o;
        if (INIT) x[(long)ch * g.ch_stride + at] = (double)canvas(y, xi, ch);
    }
}

// Seamless cloning (Perez et al. 2003) with the source already placed on the canvas: for a region pixel p,
//     b_p = sum over q in {N,S,W,E} of v_pq + sum over q outside the region of T_q
// with v_pq = S_p - S_q (MIXED false), or whichever of T_p - T_q and S_p - S_q is larger in magnitude (MIXED
// true; ties take the source).  Integers throughout: exact in any order.  The host has checked that the region
// does not touch the canvas's outer rows or columns, so every neighbour of a region pixel exists.
// init: 0 leave x, 1 x := T, 2 x := S inside the region (0 outside).  grid = (ceil(W / kBlock), local_rows).
template <bool MIXED, typename U>
__global__ void __launch_bounds__(kBlock)
k_blend_clone_rhs(double *__restrict__ b, double *__restrict__ x, BlendMask r, U src, U tgt, int C, int init)
{
    const Geom &g = r.g;
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    const int l = blockIdx.y;
    if (xi >= g.W) return;
    const int y = g.y0 + l;
    const long at = row_off(g, l, (xi + y) & 1) + (xi >> 1);
    if (!r.mask[at]) {
        for (int ch = 0; ch < C; ++ch) {
            b[(long)ch * g.ch_stride + at] = 0.0;
            if (init) x[(long)ch * g.ch_stride + at] = 0.0;
        }
        return;
    }
    const bool out[4] = {!r.at(l - 1, xi), !r.at(l + 1, xi), !r.at(l, xi - 1), !r.at(l, xi + 1)};
    const int dy[4] = {-1, 1, 0, 0}, dx[4] = {0, 0, -1, 1};
    for (int ch = 0; ch < C; ++ch) {
        const int sp = src(y, xi, ch), tp = tgt(y, xi, ch);
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tq = tgt(y + dy[k], xi + dx[k], ch);
            int v = sp - (int)src(y + dy[k], xi + dx[k], ch);
            if (MIXED) {
                const int vt = tp - tq;
                v = abs(vt) > abs(v) ? vt : v;
            }
            acc += v + (out[k] ? tq : 0);
        }
        b[(long)ch * g.ch_stride + at] = (double)acc;
        if (init) x[(long)ch * g.ch_stride + at] = (double)(init == 1 ? tp : sp);
    }
}

// Composite epilogue over the OWNED rows: out(y,x)[ch] = uchar(max(min(x,255),0)) inside the region,
// canvas(y,x)[ch] outside.  canvas / out: accessors by image row.  grid = (ceil(W / kBlock), owned rows).
template <typename U, typename O>
__global__ void __launch_bounds__(kBlock)
k_blend_composite(const double *__restrict__ x, BlendMask r, U canvas, O out, int C)
{
    const Geom &g = r.g;
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    if (xi >= g.W) return;
    const int l = g.own_lo + (int)blockIdx.y;
    const long at = row_off(g, l, (xi + g.y0 + l) & 1) + (xi >> 1);
    const bool in = r.mask[at] != 0;
    const int y = g.y0 + l;
    for (int ch = 0; ch < C; ++ch) {
        if (in) {
            double v = x[(long)ch * g.ch_stride + at];
            v = v < 255.0 ? v : 255.0;
            v = v > 0.0 ? v : 0.0;
            out(y, xi, ch) = (uint8_t)v;
        } else {
            out(y, xi, ch) = canvas(y, xi, ch);
        }
    }
}

}  // namespace ccp
