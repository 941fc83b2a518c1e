// ccp_grid_mask.hpp — ccp_grid_set_mask_device's one pass (include/ccp_gs.h): the region of a Dirichlet-mask grid from
// a strided H x W view of the whole canvas (non-zero = inside) into the handle's colour-split mask bytes, the two
// mask_edge rows, the count of owned unknowns and the verdict "the region touches the canvas's outer rows or columns".
//
// One launch, grid = (ceil(pitch / kBlock), local_rows + 4).  As in the gather / scatter kernels (ccp_grid_io.hpp) a
// lane owns the pixel pair (2j, 2j+1) of one row; j runs to the pitch, so the padding of every half-row is written 0
// as the host twin writes it.  blockIdx.y selects the work:
//   [0, local_rows)      local row l: both colour half-rows; owned rows count their set pixels (one atomic per wave);
//   local_rows, +1       the image rows y0 - 1 and y0 + local_rows into mask_edge (0 where the row does not exist);
//   local_rows + 2       rows 0 and H - 1 of the canvas: any set pixel raises the border flag;
//   local_rows + 3       columns 0 and W - 1, grid-stride over the rows: likewise.
// So a row block dereferences its local rows, one row either side, and the four border lines of the whole view.
#pragma once

#include "ccp_grid_io.hpp"

namespace ccp {

// counters[0]: owned unknowns, counters[1]: != 0 when the region touches the border (both cleared on the stream before)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_mask_split(View<const T> m, unsigned char *__restrict__ split, unsigned char *__restrict__ edge, Geom g,
             unsigned long long *__restrict__ counters)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int x0 = 2 * j, x1 = x0 + 1;
    const int r = blockIdx.y;
    if (r < g.local_rows) {
        const int y = g.y0 + r;
        const bool in0 = x0 < g.W && m(y, x0, 0) != T(0);
        const bool in1 = x1 < g.W && m(y, x1, 0) != T(0);
        if (j < g.pitch) {
            split[row_off(g, r, y & 1) + j] = in0;
            split[row_off(g, r, (y + 1) & 1) + j] = in1;
        }
        if (r >= g.own_lo && r < g.own_hi) {
            const int n = __popcll(__ballot(in0)) + __popcll(__ballot(in1));
            if (n && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (unsigned long long)n);
        }
        return;
    }
    const int k = r - g.local_rows;
    if (k < 2) {
        const int y = k == 0 ? g.y0 - 1 : g.y0 + g.local_rows;
        const bool there = y >= 0 && y < g.H;
        if (x0 < g.W) edge[(long)k * g.W + x0] = there && m(y, x0, 0) != T(0);
        if (x1 < g.W) edge[(long)k * g.W + x1] = there && m(y, x1, 0) != T(0);
        return;
    }
    bool any = false;
    if (k == 2) {
        for (int x = x0; x <= x1; ++x)
            if (x < g.W) any |= m(0, x, 0) != T(0) || m(g.H - 1, x, 0) != T(0);
    } else {
        for (long y = j; y < g.H; y += (long)gridDim.x * kBlock) any |= m((int)y, 0, 0) != T(0) || m((int)y, g.W - 1, 0) != T(0);
    }
    if (__ballot(any) && (threadIdx.x & 63) == 0) atomicOr(&counters[1], 1ull);
}

}  // namespace ccp
