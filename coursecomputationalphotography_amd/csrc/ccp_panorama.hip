// ccp_panorama.hip — C ABI of lab8's panorama merge on device views (include/ccp_gs.h): argument checks and launches of
// the kernels of ccp_panorama.hpp.  Free functions: no handle, no allocation, no host synchronisation.
#include "ccp_panorama.hpp"
#include "ccp_view_check.hpp"

using namespace ccp;

namespace {

constexpr unsigned kU8 = 1u << CCP_DTYPE_U8;
constexpr unsigned kF32 = 1u << CCP_DTYPE_F32;

template <typename T>
View<T> view_of(const ccp_device_array *a)
{
    return View<T>{static_cast<T *>(const_cast<void *>(a->data)), (long)a->stride_n, (long)a->stride_y, (long)a->stride_x,
                   (long)a->stride_c};
}

int bind_device(int device, int W, int H)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return CCP_ERR_NO_DEVICE;
    if (device < 0 || device >= count || W < 1 || H < 1) return CCP_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) return CCP_ERR_NO_DEVICE;
    return CCP_OK;
}

// the state's own refusals: four output views of the stated extents, one or three channels
int check_state(int device, const ccp_panorama_state *s)
{
    if (!s || s->reserved != 0 || (s->channels != 1 && s->channels != 3)) return CCP_ERR_BAD_ARG;
    CCP_TRY(bind_device(device, s->width, s->height));
    const long H = s->height, W = s->width, C = s->channels;
    CCP_TRY(check_view_on(device, s->dx, kF32, true, 1, H, W, C));
    CCP_TRY(check_view_on(device, s->dy, kF32, true, 1, H, W, C));
    CCP_TRY(check_view_on(device, s->raw, kU8, true, 1, H, W, C));
    return check_view_on(device, s->mask, kU8, true, 1, H, W, 1);
}

}  // namespace

extern "C" {

int ccp_mask_erode_cross_device(int32_t device, void *hip_stream, int32_t width, int32_t height, const ccp_device_array *in,
                                const ccp_device_array *out, int32_t times)
try {
    CCP_TRY(bind_device(device, width, height));
    if (times < 1 || times > kErodeMax) return CCP_ERR_BAD_ARG;
    CCP_TRY(check_view_on(device, in, kU8, false, 1, height, width, 1));
    CCP_TRY(check_view_on(device, out, kU8, true, 1, height, width, 1));
    const dim3 grid((unsigned)((width + kErodeTx - 1) / kErodeTx), (unsigned)((height + kErodeTy - 1) / kErodeTy));
    hipLaunchKernelGGL(k_pano_erode, grid, dim3(kBlock), 0, static_cast<hipStream_t>(hip_stream), view_of<const uint8_t>(in),
                       view_of<uint8_t>(out), width, height, times);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_panorama_begin_device(int32_t device, void *hip_stream, const ccp_panorama_state *s, const ccp_device_array *img0,
                              const ccp_device_array *mask0)
try {
    CCP_TRY(check_state(device, s));
    const int W = s->width, H = s->height;
    CCP_TRY(check_view_on(device, img0, kU8, false, 1, H, W, s->channels));
    CCP_TRY(check_view_on(device, mask0, kU8, false, 1, H, W, 1));
    const dim3 grid((unsigned)((W + kBlock - 1) / kBlock), (unsigned)H);
    const auto stream = static_cast<hipStream_t>(hip_stream);
    if (s->channels == 3)
        hipLaunchKernelGGL(k_pano_begin<3>, grid, dim3(kBlock), 0, stream, view_of<const uint8_t>(img0), view_of<const uint8_t>(mask0),
                           view_of<float>(s->dx), view_of<float>(s->dy), view_of<uint8_t>(s->raw), view_of<uint8_t>(s->mask), W, H);
    else
        hipLaunchKernelGGL(k_pano_begin<1>, grid, dim3(kBlock), 0, stream, view_of<const uint8_t>(img0), view_of<const uint8_t>(mask0),
                           view_of<float>(s->dx), view_of<float>(s->dy), view_of<uint8_t>(s->raw), view_of<uint8_t>(s->mask), W, H);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_panorama_add_device(int32_t device, void *hip_stream, const ccp_panorama_state *s, const ccp_device_array *img,
                            const ccp_device_array *outer, const ccp_device_array *inner)
try {
    CCP_TRY(check_state(device, s));
    const int W = s->width, H = s->height;
    CCP_TRY(check_view_on(device, img, kU8, false, 1, H, W, s->channels));
    CCP_TRY(check_view_on(device, outer, kU8, false, 1, H, W, 1));
    CCP_TRY(check_view_on(device, inner, kU8, false, 1, H, W, 1));
    const dim3 grid((unsigned)((H + kPanoRows - 1) / kPanoRows));
    const auto stream = static_cast<hipStream_t>(hip_stream);
    if (s->channels == 3)
        hipLaunchKernelGGL(k_pano_add<3>, grid, dim3(kBlock), 0, stream, view_of<const uint8_t>(img), view_of<const uint8_t>(outer),
                           view_of<const uint8_t>(inner), view_of<float>(s->dx), view_of<float>(s->dy), view_of<uint8_t>(s->raw),
                           view_of<uint8_t>(s->mask), W, H);
    else
        hipLaunchKernelGGL(k_pano_add<1>, grid, dim3(kBlock), 0, stream, view_of<const uint8_t>(img), view_of<const uint8_t>(outer),
                           view_of<const uint8_t>(inner), view_of<float>(s->dx), view_of<float>(s->dy), view_of<uint8_t>(s->raw),
                           view_of<uint8_t>(s->mask), W, H);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
} CCP_ABI_CATCH

int ccp_panorama_finish_device(int32_t device, void *hip_stream, const ccp_panorama_state *s)
try {
    CCP_TRY(check_state(device, s));
    const int W = s->width, H = s->height;
    if (W < 2 || H < 2) return CCP_OK;                   // no pixel with y < H-1 and x < W-1
    const dim3 grid((unsigned)((W - 1 + kBlock - 1) / kBlock), (unsigned)(H - 1));
    const auto stream = static_cast<hipStream_t>(hip_stream);
    if (s->channels == 3)
        hipLaunchKernelGGL(k_pano_finish<3>, grid, dim3(kBlock), 0, stream, view_of<float>(s->dx), view_of<float>(s->dy),
                           view_of<const uint8_t>(s->raw), view_of<const uint8_t>(s->mask), W, H);
    else
        hipLaunchKernelGGL(k_pano_finish<1>, grid, dim3(kBlock), 0, stream, view_of<float>(s->dx), view_of<float>(s->dy),
                           view_of<const uint8_t>(s->raw), view_of<const uint8_t>(s->mask), W, H);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"
