// ccp_grid_io.hip — what moves images in and out of a grid handle (include/ccp_gs.h): host and device rows, right-hand
// sides from gradient fields and image stacks, u8 stores and loads, region blends, clones and composites, masks.
// Every image-shaped input or output is read through a strided view (ccp_grid_io.hpp; the blends' kernels are in
// ccp_grid_blend.hpp, the mask's in ccp_grid_mask.hpp).  The ccp_grid_*_device calls pass views of the caller's device
// arrays; nothing is staged, allocated or waited for.  Their host twins stage into device memory, launch the same kernels
// on views of the staging buffers, and wait.
#include "ccp_grid_handle.hpp"
#include "ccp_grid_io.hpp"
#include "ccp_grid_blend.hpp"
#include "ccp_grid_mask.hpp"
#include "ccp_view_check.hpp"

#include <algorithm>
#include <vector>

using namespace ccp;

// ---- what ccp_grid_weighted.hip calls too (ccp_grid_handle.hpp) ----
namespace ccp {

int check_view(const ccp_grid *g, const ccp_device_array *a, unsigned dtypes, bool output, long n, long y, long x, long c)
{
    return check_view_on(g->desc.device, a, dtypes, output, n, y, x, c);
}

// a caller's view (or none) as the weighted handle's operator kernels read it
ImageView image_view(const ccp_device_array *a, double dflt)
{
    if (!a) return ImageView{nullptr, 0, 0, 0, 0, dflt};
    return ImageView{a->data, (long)a->stride_y, (long)a->stride_x, (long)a->stride_c, a->dtype, dflt};
}

// one lane per pixel of a row: ceil(W / kBlock) blocks by `rows` (by `channels` where a lane serves one channel)
dim3 pixel_grid(const ccp_grid *g, int rows, int channels)
{
    return dim3((unsigned)((g->desc.width + kBlock - 1) / kBlock), (unsigned)rows, (unsigned)channels);
}

}  // namespace ccp

namespace {

template <typename T>
View<T> view_of(const ccp_device_array *a)
{
    return View<T>{static_cast<T *>(const_cast<void *>(a->data)), (long)a->stride_n, (long)a->stride_y, (long)a->stride_x,
                   (long)a->stride_c};
}

bool single_block(const ccp_grid *g) { return !(g->ghost_top || g->ghost_bottom || g->desc.row_count != g->desc.height); }

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

}  // namespace

extern "C" {

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

}  // extern "C"

// Library-internal twin of ccp_grid_set_mask_host for a mask that is already on the device in the grid's layout
// (the region recognition builds it there: ccp_csr.hip).  Asynchronous on the handle's stream.
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
