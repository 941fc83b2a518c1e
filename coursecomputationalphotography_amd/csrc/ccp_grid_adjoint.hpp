// ccp_grid_adjoint.hpp — the backward pass of a weighted grid solve (include/ccp_gs.h, ccp_grid_adjoint_begin_device and
// ccp_grid_weighted_adjoint_device), hand-written for gfx950: the pass that loads the adjoint right-hand side and the pass
// that turns the forward solution u and the adjoint solution v into the gradients of every input.
//
// Mathematics.  The forward solve minimises E(u) of CCP_GRID_WEIGHTED over the free pixels; its output is the composite
// u.  With G = dL/du, v solves A_FF v_F = G_F on the free pixels (the operator is symmetric: one more solve on the same
// handle) and is 0 on fixed and dead pixels.  Per channel, s_x = v(x+1,y) - v(x,y), r_x = gx - (u(x+1,y) - u(x,y)), s_y and
// r_y likewise to the south:
//     dL/dwx = sum_c s_x r_x      dL/dgx = wx s_x          dL/dlambda = sum_c v (f - u)   (free pixels; 0 at fixed ones)
//     dL/dwy = sum_c s_y r_y      dL/dgy = wy s_y          dL/df      = lambda v          (free pixels; 0 at fixed ones)
//     dL/dvalues = G + wN vN + wW vW + wE vE + wS vS at a fixed pixel (absent edges skipped, the ORIGINAL weights), 0 at free ones
// The edge formulas hold unchanged on edges with fixed ends because v is 0 there.
//
// Operation order (fp64 throughout, inputs widened exactly, nothing contracted to an fma; tests/adjoint_helpers.py is the
// same in numpy).  v is the handle's x, read as +0.0 at a fixed pixel whatever it holds there.  One thread per pixel (x,y):
//   east edge, x + 1 < W, per channel in channel order:   s = vE - v;  r = gx - (uE - u);  g_gx = w * s;  acc += s * r
//       (acc from +0.0; w = wx(x,y));  g_wx = acc.  x = W - 1: g_wx = g_gx = +0.0.
//   south edge, y + 1 < H: the same with vS, uS, gy, w = wy(x,y), g_gy, g_wy.  y = H - 1: g_wy = g_gy = +0.0.
//   free pixel, per channel:  g_f = lambda * v;  accl += v * (f - u)  (accl from +0.0);  g_values = +0.0;  g_lambda = accl.
//   fixed pixel, per channel: t = G; t += wN*vN; t += wW*vW; t += wE*vE; t += wS*vS (absent edges skipped); g_values = t;
//       g_f = +0.0;  g_lambda = +0.0.
// A float32 output is the fp64 value rounded to nearest once.  A missing gx, gy or f reads +0.0, a missing wx or wy 1.0, a
// missing lambda +0.0, a missing mask "no pixel is fixed".
//
// Memory.  x is read in the handle's colour-split layout (w_at); every other array through AdjIn / AdjOut, the strided
// element addressing of ccp_grid_io.hpp's View with the dtype picked at run time (a wave-uniform branch) so that one
// kernel serves every combination of dtypes and of requested outputs.  Lanes run along x: on the split planes a wave
// reads two runs of 32 contiguous doubles, on a natural-order view one row segment.  The pass is bandwidth-bound; a
// pixel's east, south, north and west neighbours are its lane neighbours' and the next rows' own loads and come from the
// cache.  No LDS, no scratch: nothing is indexed at run time but global memory.
//
// The two pixel bodies are plain functions of (args, x, y) so that tests/cpp/adjoint_host_check.cpp can run this very
// source on the host under sanitizers (CCP_ADJOINT_HOST: no HIP, w_at and kBlock pasted in as text).
#pragma once

#ifdef CCP_ADJOINT_HOST
#include <cstdint>
#define CCP_ADJ_FN inline
#include "adjoint_host_real.inc"       // kBlock and w_at, as text from the real headers
#else
#include "ccp_grid_stencil.hpp"        // w_at
#define CCP_ADJ_FN __host__ __device__ __forceinline__
#endif

namespace ccp {

constexpr int kAdjU8 = 1, kAdjF32 = 2, kAdjF64 = 3;      // CCP_DTYPE_*

// A read-only H x W (x C) view: element (y, x, c) at p + y*sy + x*sx + c*sc elements of `dtype`; p == nullptr: absent.
struct AdjIn {
    const void *p;
    long sy, sx, sc;
    int dtype;
};

CCP_ADJ_FN double adj_load(const AdjIn &a, int y, int x, int c, double absent)
{
    if (!a.p) return absent;
    const long i = (long)y * a.sy + (long)x * a.sx + (long)c * a.sc;
    if (a.dtype == kAdjF64) return static_cast<const double *>(a.p)[i];
    if (a.dtype == kAdjF32) return (double)static_cast<const float *>(a.p)[i];
    return (double)static_cast<const unsigned char *>(a.p)[i];
}

// An output view, F32 or F64; p == nullptr: not asked for.
struct AdjOut {
    void *p;
    long sy, sx, sc;
    int dtype;
};

CCP_ADJ_FN void adj_store(const AdjOut &a, int y, int x, int c, double v)
{
    if (!a.p) return;
    const long i = (long)y * a.sy + (long)x * a.sx + (long)c * a.sc;
    if (a.dtype == kAdjF64)
        static_cast<double *>(a.p)[i] = v;
    else
        static_cast<float *>(a.p)[i] = (float)v;
}

struct AdjointArgs {
    const double *v;             // the handle's x: C planes `ch_stride` doubles apart, colour-split (w_at)
    long pitch, ch_stride;
    int W, H, C;
    AdjIn u, grad, gx, gy, f, wx, wy, lam, fixed;
    AdjOut g_wx, g_wy, g_lam, g_gx, g_gy, g_f, g_val;
};

CCP_ADJ_FN bool adj_fixed(const AdjIn &m, int y, int x) { return m.p && adj_load(m, y, x, 0, 0.0) != 0.0; }

// A view at one pixel: the address of its channel 0 there and the step to the next channel, in bytes.  adjoint_pixel
// forms these once, before its channel loop, so that the loop carries one address per view instead of the view's strides.
struct AdjCursor {
    const char *p;               // nullptr: absent
    long step;
    int dtype;
};

CCP_ADJ_FN long adj_size(int dtype) { return dtype == kAdjF64 ? 8 : dtype == kAdjF32 ? 4 : 1; }

CCP_ADJ_FN AdjCursor adj_cursor(const void *p, long sy, long sx, long sc, int dtype, int y, int x)
{
    if (!p) return AdjCursor{nullptr, 0, 0};
    const long es = adj_size(dtype);
    return AdjCursor{static_cast<const char *>(p) + ((long)y * sy + (long)x * sx) * es, sc * es, dtype};
}

CCP_ADJ_FN AdjCursor adj_cursor(const AdjIn &a, int y, int x) { return adj_cursor(a.p, a.sy, a.sx, a.sc, a.dtype, y, x); }
CCP_ADJ_FN AdjCursor adj_cursor(const AdjOut &a, int y, int x) { return adj_cursor(a.p, a.sy, a.sx, a.sc, a.dtype, y, x); }

CCP_ADJ_FN double adj_load(const AdjCursor &k, int c, double absent)
{
    if (!k.p) return absent;
    const char *q = k.p + (long)c * k.step;
    if (k.dtype == kAdjF64) return *reinterpret_cast<const double *>(q);
    if (k.dtype == kAdjF32) return (double)*reinterpret_cast<const float *>(q);
    return (double)*reinterpret_cast<const unsigned char *>(q);
}

CCP_ADJ_FN void adj_store(const AdjCursor &k, int c, double v)
{
    if (!k.p) return;
    char *q = const_cast<char *>(k.p) + (long)c * k.step;
    if (k.dtype == kAdjF64)
        *reinterpret_cast<double *>(q) = v;
    else
        *reinterpret_cast<float *>(q) = (float)v;
}

// Every gradient of pixel (x, y): its east edge, its south edge, its pixel terms.  P: a pointer to AdjointArgs -- in the
// kernel one into the kernel-argument segment (its address space is part of P), so the views are fetched member by member.
#define CCP_ADJ_IN(a, m) AdjIn{(a)->m.p, (a)->m.sy, (a)->m.sx, (a)->m.sc, (a)->m.dtype}
#define CCP_ADJ_OUT(a, m) AdjOut{(a)->m.p, (a)->m.sy, (a)->m.sx, (a)->m.sc, (a)->m.dtype}
template <typename P>
CCP_ADJ_FN void adjoint_pixel(P a, int x, int y)
{
    const bool has_e = x + 1 < a->W, has_s = y + 1 < a->H;
    const bool east = has_e && (a->g_wx.p || a->g_gx.p), south = has_s && (a->g_wy.p || a->g_gy.p);
    const bool fp = adj_fixed(CCP_ADJ_IN(a, fixed), y, x);
    const bool at_fixed = fp && a->g_val.p;                               // the four-neighbour sum is wanted here
    const bool need_e = east || (at_fixed && has_e), need_s = south || (at_fixed && has_s);
    const bool need_n = at_fixed && y >= 1, need_w = at_fixed && x >= 1;
    const bool f_e = need_e && adj_fixed(CCP_ADJ_IN(a, fixed), y, x + 1), f_s = need_s && adj_fixed(CCP_ADJ_IN(a, fixed), y + 1, x);
    const bool f_n = need_n && adj_fixed(CCP_ADJ_IN(a, fixed), y - 1, x), f_w = need_w && adj_fixed(CCP_ADJ_IN(a, fixed), y, x - 1);
    const double w_e = need_e ? adj_load(CCP_ADJ_IN(a, wx), y, x, 0, 1.0) : 0.0, w_s = need_s ? adj_load(CCP_ADJ_IN(a, wy), y, x, 0, 1.0) : 0.0;
    const double w_n = need_n ? adj_load(CCP_ADJ_IN(a, wy), y - 1, x, 0, 1.0) : 0.0, w_w = need_w ? adj_load(CCP_ADJ_IN(a, wx), y, x - 1, 0, 1.0) : 0.0;
    const bool pixel = !fp && (a->g_f.p || a->g_lam.p);
    const double lam = pixel && a->g_f.p ? adj_load(CCP_ADJ_IN(a, lam), y, x, 0, 0.0) : 0.0;
    const bool need_u = east || south || (pixel && a->g_lam.p);
    // v of the pixel and of the neighbours that are read: nullptr stands for +0.0 (a fixed pixel, or not needed)
    const long at = w_at(a->pitch, x, y);
    const double *v_c = fp ? nullptr : a->v + at;
    const double *v_e = need_e && !f_e ? a->v + w_at(a->pitch, x + 1, y) : nullptr;
    const double *v_s = need_s && !f_s ? a->v + w_at(a->pitch, x, y + 1) : nullptr;
    const double *v_n = need_n && !f_n ? a->v + w_at(a->pitch, x, y - 1) : nullptr;
    const double *v_w = need_w && !f_w ? a->v + w_at(a->pitch, x - 1, y) : nullptr;
    const AdjCursor none{nullptr, 0, 0};
    const AdjCursor u_c = need_u ? adj_cursor(CCP_ADJ_IN(a, u), y, x) : none;
    const AdjCursor u_e = east ? adj_cursor(CCP_ADJ_IN(a, u), y, x + 1) : none, u_s = south ? adj_cursor(CCP_ADJ_IN(a, u), y + 1, x) : none;
    const AdjCursor k_gx = east ? adj_cursor(CCP_ADJ_IN(a, gx), y, x) : none, k_gy = south ? adj_cursor(CCP_ADJ_IN(a, gy), y, x) : none;
    const AdjCursor k_f = pixel && a->g_lam.p ? adj_cursor(CCP_ADJ_IN(a, f), y, x) : none;
    const AdjCursor k_grad = at_fixed ? adj_cursor(CCP_ADJ_IN(a, grad), y, x) : none;
    const AdjCursor o_gx = adj_cursor(CCP_ADJ_OUT(a, g_gx), y, x), o_gy = adj_cursor(CCP_ADJ_OUT(a, g_gy), y, x), o_f = adj_cursor(CCP_ADJ_OUT(a, g_f), y, x);
    const AdjCursor o_val = adj_cursor(CCP_ADJ_OUT(a, g_val), y, x);
    double acc_x = 0.0, acc_y = 0.0, acc_l = 0.0;
    for (int c = 0; c < a->C; ++c) {
        const long ch = (long)c * a->ch_stride;
        const double v = v_c ? v_c[ch] : 0.0, ve = v_e ? v_e[ch] : 0.0, vs = v_s ? v_s[ch] : 0.0;
        const double u = adj_load(u_c, c, 0.0);
        if (east) {
            const double s = ve - v;
            const double r = adj_load(k_gx, c, 0.0) - (adj_load(u_e, c, 0.0) - u);
            adj_store(o_gx, c, w_e * s);
            acc_x += s * r;
        } else {
            adj_store(o_gx, c, 0.0);
        }
        if (south) {
            const double s = vs - v;
            const double r = adj_load(k_gy, c, 0.0) - (adj_load(u_s, c, 0.0) - u);
            adj_store(o_gy, c, w_s * s);
            acc_y += s * r;
        } else {
            adj_store(o_gy, c, 0.0);
        }
        if (!fp) {
            adj_store(o_f, c, lam * v);
            if (pixel && a->g_lam.p) acc_l += v * (adj_load(k_f, c, 0.0) - u);
            adj_store(o_val, c, 0.0);
        } else {
            adj_store(o_f, c, 0.0);
            if (at_fixed) {
                double t = adj_load(k_grad, c, 0.0);
                if (need_n) t += w_n * (v_n ? v_n[ch] : 0.0);
                if (need_w) t += w_w * (v_w ? v_w[ch] : 0.0);
                if (has_e) t += w_e * ve;
                if (has_s) t += w_s * vs;
                adj_store(o_val, c, t);
            }
        }
    }
    adj_store(CCP_ADJ_OUT(a, g_wx), y, x, 0, acc_x);
    adj_store(CCP_ADJ_OUT(a, g_wy), y, x, 0, acc_y);
    adj_store(CCP_ADJ_OUT(a, g_lam), y, x, 0, acc_l);
}

// ccp_grid_adjoint_begin_device, pixel (x, y) of every channel: b := G on a free live pixel (d != 0: a fixed pixel's d
// is 0 as a dead one's) and +0.0 elsewhere; x := +0.0.
CCP_ADJ_FN void adjoint_begin_pixel(double *b, double *xo, const double *d, long pitch, long ch_stride, int C, const AdjIn &grad, int x, int y)
{
    const long at = w_at(pitch, x, y);
    const bool live = d[at] != 0.0;
    for (int c = 0; c < C; ++c) {
        b[(long)c * ch_stride + at] = live ? adj_load(grad, y, x, c, 0.0) : 0.0;
        xo[(long)c * ch_stride + at] = 0.0;
    }
}

#ifndef CCP_ADJOINT_HOST
// grid = (ceil(W / kBlock), H) for both
// The sixteen views are 640 bytes of kernel arguments, more than a wave's scalar registers hold.  Taken as an ordinary
// by-value argument they are all fetched at the kernel's entry and most of them spilled at once; read through the
// kernel-argument segment pointer, made opaque to the optimiser, each member is fetched -- by a scalar load, as before --
// where adjoint_pixel uses it.
typedef const __attribute__((address_space(4))) AdjointArgs *AdjointKernArgs;

static __global__ void __launch_bounds__(kBlock) k_weighted_adjoint(AdjointArgs)
{
    AdjointKernArgs a = (AdjointKernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x < a->W) adjoint_pixel(a, x, y);
}

static __global__ void __launch_bounds__(kBlock)
k_adjoint_begin(double *__restrict__ b, double *__restrict__ xo, const double *__restrict__ d, long pitch, long ch_stride, int W, int C, AdjIn grad)
{
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x < W) adjoint_begin_pixel(b, xo, d, pitch, ch_stride, C, grad, x, y);
}
#endif

}  // namespace ccp
