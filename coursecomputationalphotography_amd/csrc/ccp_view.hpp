// ccp_view.hpp — View<T>, the strided accessor of every image-shaped kernel argument (ccp_grid_io.hpp explains it): four
// element strides over a caller's device array or a staging buffer.  No kernels here, so that more than one translation
// unit may include it.
#pragma once

#include "ccp_common.hpp"

namespace ccp {

template <typename T>
struct View {
    T *p;
    long sn, sy, sx, sc; // strides in elements
    __device__ __forceinline__ T &operator()(int y, int x, int c) const { return p[(long)y * sy + (long)x * sx + (long)c * sc]; }
    __device__ __forceinline__ T &at(int n, int y, int x, int c) const
    {
        return p[(long)n * sn + (long)y * sy + (long)x * sx + (long)c * sc];
    }
};

}  // namespace ccp
