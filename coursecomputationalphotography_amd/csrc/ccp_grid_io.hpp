// ccp_grid_io.hpp — device hand-off of a grid handle (include/ccp_gs.h, the ccp_grid_*_device calls): the element
// accessors the assembly, clone, composite and u8 kernels read through, and the gather / scatter kernels between a
// strided natural-order view and the split colour layout of x and b.
//
// Accessors.  Every image-shaped input or output of a kernel is read as acc(y, x, c) (acc.at(n, y, x, c) for an
// image stack) with y the IMAGE row.  View<T> is the one accessor: four element strides over a caller's device array
// (the _device calls) or over a staging buffer of a host entry point, whose packed row window (interleaved W x C
// rows from image row `ya` on) is the strides (plane, W * C, C, 1) with the base moved back by `ya` rows.
//
// Gather / scatter.  One lane owns the pixel pair (2j, 2j+1) of one row for every channel: pixel 2j has colour
// y&1 and pixel 2j+1 colour (y+1)&1, both at half-column j, so a wave writes (or reads) 64 contiguous doubles of
// each colour half-row.  KIND picks how the natural side is read: kPairs when stride_x == 1 and a pair is one
// aligned 2-element vector (channel-planar C x H x W, and any C = 1 row), kRgb when the view is interleaved with
// C == 3 (the 6 values of a pair are contiguous: three 2-element vectors), kGeneral for any other strides.
//
// Below them: the layout conversion of the host row calls (k_convert) and the assembly, u8 store and u8 load kernels.
// Included by ccp_grid_io.hip alone (k_io_label_check is neither a template nor static).
#pragma once

#include "ccp_grid_stencil.hpp"
#include "ccp_view.hpp"          // View<T>, the one accessor

#include <cstdint>

namespace ccp {

// the pin values of k_assemble_rhs, passed by value
struct Pins {
    int v[kMaxChannels];
    __device__ __forceinline__ int operator[](int c) const { return v[c]; }
};

enum IoKind { kGeneral = 0, kPairs = 1, kRgb = 3 };

template <typename T>
struct Vec2;
template <>
struct Vec2<double> { using type = double2; };
template <>
struct Vec2<float> { using type = float2; };

// The pair (2j, 2j+1) of channel c in row y: v[0], v[1] (v[1] only when `two`).
template <int KIND, typename T>
__device__ __forceinline__ void load_pair(const View<const T> &a, int y, int x0, int c, bool two, T (&v)[2])
{
    if (KIND == kPairs && two) {
        const auto t = *reinterpret_cast<const typename Vec2<T>::type *>(&a(y, x0, c));
        v[0] = t.x;
        v[1] = t.y;
    } else {
        v[0] = a(y, x0, c);
        v[1] = two ? a(y, x0 + 1, c) : T(0);
    }
}

template <int KIND, typename T>
__device__ __forceinline__ void store_pair(const View<T> &a, int y, int x0, int c, bool two, const T (&v)[2])
{
    if (KIND == kPairs && two) {
        typename Vec2<T>::type t;
        t.x = v[0];
        t.y = v[1];
        *reinterpret_cast<typename Vec2<T>::type *>(&a(y, x0, c)) = t;
    } else {
        a(y, x0, c) = v[0];
        if (two) a(y, x0 + 1, c) = v[1];
    }
}

// Natural -> split for all channels: image rows [first_row, first_row + gridDim.y) from view rows 0.. (array row r =
// image row first_row + r).  MASKED: pixels outside the region are written 0 (the mask grid's zero_unmasked, fused).
// grid = (ceil(ceil(W/2) / kBlock), n_rows).
template <int KIND, bool MASKED, typename T>
__global__ void __launch_bounds__(kBlock)
k_io_scatter(double *__restrict__ split, View<const T> in, const unsigned char *__restrict__ mask, Geom g, int first_row, int C)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int r = blockIdx.y;
    const int x0 = 2 * j;
    if (x0 >= g.W) return;
    const bool two = x0 + 1 < g.W;
    const int y = first_row + r;
    const int l = y - g.y0;
    const long at0 = row_off(g, l, y & 1) + j;          // pixel 2j
    const long at1 = row_off(g, l, (y + 1) & 1) + j;    // pixel 2j+1
    bool in0 = true, in1 = true;
    if (MASKED) {
        in0 = mask[at0] != 0;
        in1 = two && mask[at1] != 0;
    }
    if (KIND == kRgb) {
        // interleaved, C == 3: the pair's six values are contiguous (2-element aligned when the host chose kRgb)
        using V2 = typename Vec2<T>::type;
        T v[6];
        const T *src = &in(r, x0, 0);
        if (two) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const V2 t = reinterpret_cast<const V2 *>(src)[k];
                v[2 * k] = t.x;
                v[2 * k + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = src[k];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            split[(long)ch * g.ch_stride + at0] = in0 ? (double)v[ch] : 0.0;
            if (two) split[(long)ch * g.ch_stride + at1] = in1 ? (double)v[3 + ch] : 0.0;
        }
        return;
    }
    for (int ch = 0; ch < C; ++ch) {
        T v[2];
        load_pair<KIND>(in, r, x0, ch, two, v);
        split[(long)ch * g.ch_stride + at0] = in0 ? (double)v[0] : 0.0;
        if (two) split[(long)ch * g.ch_stride + at1] = in1 ? (double)v[1] : 0.0;
    }
}

// Split -> natural for all channels (T = float rounds to nearest).  grid as k_io_scatter.
template <int KIND, typename T>
__global__ void __launch_bounds__(kBlock)
k_io_gather(const double *__restrict__ split, View<T> out, Geom g, int first_row, int C)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int r = blockIdx.y;
    const int x0 = 2 * j;
    if (x0 >= g.W) return;
    const bool two = x0 + 1 < g.W;
    const int y = first_row + r;
    const int l = y - g.y0;
    const long at0 = row_off(g, l, y & 1) + j;
    const long at1 = row_off(g, l, (y + 1) & 1) + j;
    if (KIND == kRgb) {
        using V2 = typename Vec2<T>::type;
        T v[6];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            v[ch] = (T)split[(long)ch * g.ch_stride + at0];
            v[3 + ch] = two ? (T)split[(long)ch * g.ch_stride + at1] : T(0);
        }
        T *dst = &out(r, x0, 0);
        if (two) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                V2 t;
                t.x = v[2 * k];
                t.y = v[2 * k + 1];
                reinterpret_cast<V2 *>(dst)[k] = t;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[k] = v[k];
        }
        return;
    }
    for (int ch = 0; ch < C; ++ch) {
        T v[2];
        v[0] = (T)split[(long)ch * g.ch_stride + at0];
        v[1] = two ? (T)split[(long)ch * g.ch_stride + at1] : T(0);
        store_pair<KIND>(out, r, x0, ch, two, v);
    }
}

// ccp_grid_assemble_from_images_device's guard: *bad := 1 if any label of the H x W view is >= n_images (*bad is
// cleared on the stream before).  grid-stride over the pixels.
__global__ void __launch_bounds__(kBlock)
k_io_label_check(View<const uint8_t> label, int W, int H, int n_images, unsigned *__restrict__ bad)
{
    const long n = (long)W * H;
    bool any = false;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        any |= label(y, x, 0) >= n_images;
    }
    if (any) atomicOr(bad, 1u);
}

// ---------------------------------------------------------------------------------------------
// Layout conversion between natural raster rows (what std::vector<double> holds in the
// reference) and the row-split colour planes.  grid = (ceil(W/kBlock), rows).
template <bool TO_SPLIT>
__global__ void __launch_bounds__(kBlock)
k_convert(double *__restrict__ split, double *__restrict__ natural, Geom g, int ch, int l_first,
          int W)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= W) return;
    const int l = l_first + r;
    const int c = (x + g.y0 + l) & 1;
    const long s = (long)ch * g.ch_stride + row_off(g, l, c) + (x >> 1);
    const long n = (long)r * W + x;
    if (TO_SPLIT) split[s] = natural[n];
    else natural[n] = split[s];
}

// ---------------------------------------------------------------------------------------------
// Poisson right-hand side ATb for all channels (PhotoMontage.cpp:563-572,579-581,592), Eigen's
// row-major sparse*dense accumulation order: gy above, gx left, -gx here, -gy here, pin.
// gx, gy: H x W x C float32 on device through accessor F (ccp_grid_io.hpp), the pins through PIN (Pins by
// value).  grid = (ceil(W/kBlock), H, C).
template <typename F, typename PIN>
__global__ void __launch_bounds__(kBlock)
k_assemble_rhs(double *__restrict__ b, Geom g, F gx, F gy, PIN constraint)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    const int y = blockIdx.y;
    const int ch = blockIdx.z;
    if (x >= g.W) return;
    double acc = 0.0;
    if (y >= 1 && x < g.W - 1) acc += 1.0 * (double)gy(y - 1, x, ch);
    if (x >= 1 && y < g.H - 1) acc += 1.0 * (double)gx(y, x - 1, ch);
    if (x < g.W - 1 && y < g.H - 1) {
        acc += -1.0 * (double)gx(y, x, ch);
        acc += -1.0 * (double)gy(y, x, ch);
    }
    if ((x | y) == 0) acc += 1.0 * (double)constraint[ch];
    const int l = y - g.y0;
    b[(long)ch * g.ch_stride + row_off(g, l, (x + y) & 1) + (x >> 1)] = acc;
}

// Gradient field + right-hand side in one pass, straight from the source images and the label
// map (BuildSolveGradientFusion, PhotoMontage.cpp:419-433): the forward differences of
// GradientAt (:399-408: integer subtraction of the label-selected image, then float) feed the
// same ATb accumulation as k_assemble_rhs, with the pin value Images[0](0,0)[ch] (:428).
// INIT: also write the composite image as the start vector (PhotoMontage.cpp:599-610).
// images: K stacked H x W x 3 u8 images (accessor IMG, image k = img.at(k, ...)), label: H x W u8 (accessor LAB).
// grid = (ceil(W/kBlock), H, 3).
template <bool INIT, typename IMG, typename LAB>
__global__ void __launch_bounds__(kBlock)
k_assemble_from_images(double *__restrict__ b, double *__restrict__ x, Geom g, IMG images, LAB label)
{
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    const int y = blockIdx.y;
    const int ch = blockIdx.z;
    if (xi >= g.W) return;
    auto pix = [&](int k, int yy, int xx) -> int { return (int)images.at(k, yy, xx, ch); };
    auto lab = [&](int yy, int xx) -> int { return (int)label(yy, xx, 0); };
    double acc = 0.0;
    if (y >= 1 && xi < g.W - 1) {                       // gy(y-1, x) of the cell above
        const int k = lab(y - 1, xi);
        acc += 1.0 * (double)(float)(pix(k, y, xi) - pix(k, y - 1, xi));
    }
    if (xi >= 1 && y < g.H - 1) {                       // gx(y, x-1) of the cell to the left
        const int k = lab(y, xi - 1);
        acc += 1.0 * (double)(float)(pix(k, y, xi) - pix(k, y, xi - 1));
    }
    if (xi < g.W - 1 && y < g.H - 1) {                  // -gx(y,x) - gy(y,x) of this cell
        const int k = lab(y, xi);
        const int here = pix(k, y, xi);
        acc += -1.0 * (double)(float)(pix(k, y, xi + 1) - here);
        acc += -1.0 * (double)(float)(pix(k, y + 1, xi) - here);
    }
    if ((xi | y) == 0) acc += 1.0 * (double)pix(0, 0, 0);
    const long at = (long)ch * g.ch_stride + row_off(g, y - g.y0, (xi + y) & 1) + (xi >> 1);
    b[at] = acc;
    if (INIT) x[at] = (double)pix(lab(y, xi), y, xi);
}

// Solve epilogue: out(y,x)[ch] = uchar(max(min(sol,255),0)) (PhotoMontage.cpp:617-626).  out: accessor OUT.
template <typename OUT>
__global__ void __launch_bounds__(kBlock)
k_store_u8(const double *__restrict__ x, Geom g, OUT out)
{
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    const int y = blockIdx.y;
    const int ch = blockIdx.z;
    if (xi >= g.W) return;
    const int l = y - g.y0;
    double v = x[(long)ch * g.ch_stride + row_off(g, l, (xi + y) & 1) + (xi >> 1)];
    v = v < 255.0 ? v : 255.0;
    v = v > 0.0 ? v : 0.0;
    out(y, xi, ch) = (uint8_t)v;
}

// Composite initial guess: x(y,x)[ch] = image(y,x)[ch] (PhotoMontage.cpp:599-610).  img: accessor IMG.
template <typename IMG>
__global__ void __launch_bounds__(kBlock)
k_load_u8(double *__restrict__ x, Geom g, IMG img)
{
    const int xi = blockIdx.x * kBlock + threadIdx.x;
    const int y = blockIdx.y;
    const int ch = blockIdx.z;
    if (xi >= g.W) return;
    const int l = y - g.y0;
    x[(long)ch * g.ch_stride + row_off(g, l, (xi + y) & 1) + (xi >> 1)] =
        (double)img(y, xi, ch);
}

}  // namespace ccp
