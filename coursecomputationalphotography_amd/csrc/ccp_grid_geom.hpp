// ccp_grid_geom.hpp — Geom, the layout of a grid handle's rows.  A plain struct without any HIP, so that the host-only
// pass planner (ccp_fused_plan.hpp) and the kernels (ccp_grid_stencil.hpp) share one definition.
#pragma once

namespace ccp {

struct Geom {
    int W, H;            // whole image
    int y0;              // image row of local row 0
    int local_rows;      // ghost_top + owned + ghost_bottom
    int own_lo, own_hi;  // owned local rows [own_lo, own_hi)
    long pitch;          // doubles per colour half-row
    long ch_stride;      // doubles per channel = local_rows*2*pitch
};

}  // namespace ccp
