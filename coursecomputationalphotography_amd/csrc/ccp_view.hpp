// ccp_view.hpp — View<T>, the strided accessor of every image-shaped kernel argument (ccp_grid_io.hpp explains it): four
// element strides over a caller's device array or a staging buffer; and ImageView, the accessor of the weighted handle's
// operator kernels, whose element type is a run-time field.  No kernels here, so that more than one translation unit may
// include it.
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

// An H x W x C array read as doubles: u8, f32 or f64 elements `sy`, `sx`, `sc` apart (0 broadcasts), or none
// (p == nullptr): `dflt` everywhere.  The dtype is uniform over a launch, so the branch costs no divergence; every
// conversion to double is exact.
struct ImageView {
    const void *p;
    long sy, sx, sc;
    int dtype;                                                             // CCP_DTYPE_*
    double dflt;
    __device__ __forceinline__ double operator()(int y, int x, int c) const
    {
        if (!p) return dflt;
        const long i = (long)y * sy + (long)x * sx + (long)c * sc;
        if (dtype == CCP_DTYPE_F64) return static_cast<const double *>(p)[i];
        if (dtype == CCP_DTYPE_F32) return (double)static_cast<const float *>(p)[i];
        return (double)static_cast<const unsigned char *>(p)[i];
    }
    // the same element of a view the caller knows to be there and of f32 (the guidance fields): one plain load
    __device__ __forceinline__ double f32(int y, int x, int c) const
    {
        return (double)static_cast<const float *>(p)[(long)y * sy + (long)x * sx + (long)c * sc];
    }
};

}  // namespace ccp
