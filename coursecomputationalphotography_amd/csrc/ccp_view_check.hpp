// ccp_view_check.hpp — the host-side refusals of a ccp_device_array (include/ccp_gs.h, "Device hand-off"), shared by
// the grid handles' _device calls (ccp_grid_io.hip, ccp_grid_weighted.hip) and the free panorama calls (ccp_panorama.hip).  Host code only.
#pragma once

#include "ccp_common.hpp"

#include <cstdint>
#include <utility>

namespace ccp {

inline size_t dtype_bytes(int dtype) { return dtype == CCP_DTYPE_U8 ? 1 : dtype == CCP_DTYPE_F32 ? 4 : dtype == CCP_DTYPE_F64 ? 8 : 0; }

// Refusals of a view of device `device`'s memory with extents (n, y, x, c), checked on the host before anything is
// enqueued.  `dtypes`: bit (1 << CCP_DTYPE_*) of every accepted dtype.  An output must not have two elements at one
// address.
inline int check_view_on(int device, const ccp_device_array *a, unsigned dtypes, bool output, long n, long y, long x, long c)
{
    if (!a || !a->data || a->reserved != 0) return CCP_ERR_BAD_ARG;
    if (a->dtype < 0 || a->dtype > 31 || !(dtypes & (1u << a->dtype))) return CCP_ERR_BAD_ARG;
    const long ext[4] = {n, y, x, c};
    const long str[4] = {(long)a->stride_n, (long)a->stride_y, (long)a->stride_x, (long)a->stride_c};
    for (int k = 0; k < 4; ++k)
        if (str[k] < 0 || ext[k] < 0) return CCP_ERR_BAD_ARG;
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, a->data) != hipSuccess) {
        (void)hipGetLastError();                            // pageable host memory: not a runtime allocation
        return CCP_ERR_BAD_ARG;
    }
    if (attr.type != hipMemoryTypeDevice || attr.isManaged || attr.device != device) return CCP_ERR_BAD_ARG;
    if (n == 0 || y == 0 || x == 0 || c == 0) return CCP_OK;
    const size_t es = dtype_bytes(a->dtype);
    unsigned long long last = 0;                            // element offset of the last element
    for (int k = 0; k < 4; ++k) last += (unsigned long long)(ext[k] - 1) * (unsigned long long)str[k];
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(a->data)) != hipSuccess) {
        (void)hipGetLastError();
        return CCP_ERR_BAD_ARG;
    }
    const unsigned long long lo = (unsigned long long)(uintptr_t)a->data, b0 = (unsigned long long)(uintptr_t)base;
    if (lo < b0 || lo - b0 + (last + 1) * es > size) return CCP_ERR_BAD_ARG;
    if (output) {
        // sorted by stride, each stride >= stride * extent of the one below (dimensions of extent 1 do not count)
        long s_[4], e_[4];
        int m = 0;
        for (int k = 0; k < 4; ++k)
            if (ext[k] > 1) {
                s_[m] = str[k];
                e_[m] = ext[k];
                ++m;
            }
        for (int i = 1; i < m; ++i)
            for (int k = i; k > 0 && s_[k] < s_[k - 1]; --k) {
                std::swap(s_[k], s_[k - 1]);
                std::swap(e_[k], e_[k - 1]);
            }
        for (int i = 0; i < m; ++i)
            if (s_[i] < (i ? s_[i - 1] * e_[i - 1] : 1)) return CCP_ERR_BAD_ARG;
    }
    return CCP_OK;
}

}  // namespace ccp
