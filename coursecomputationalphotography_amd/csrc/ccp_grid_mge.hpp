// ccp_grid_mge.hpp — the two kernels of the enqueue-only multigrid PCG (include/ccp_gs.h:
// ccp_grid_mg_conjugate_gradient_enqueue), hand-written for gfx950.  The recurrence, its kernels and its launch geometry
// are the synchronous call's (ccp_grid_mg.hpp, ccp_cg.hpp, ccp_grid_mgn.hpp); what the host does there with copies is done
// here on the device:
//
//   k_mge_init     the C CgStates of a solve, where the synchronous call uploads them from the host
//   k_mge_report   the report of C channels into a strided view of device memory, where the synchronous call reads the
//                  states back and fills ccp_gs_report
//
// Both are one workgroup of plain vector stores, one lane per channel (C <= kMaxChannels).
#pragma once

#include "ccp_grid_mgn.hpp"

namespace ccp {

constexpr int kMgeReportFields = 6;   // iterations, converged, last_l1_step, b_mean, x_mean, reserved

// st[c] := a state about to start (active, every count and scalar 0: what pcg_loop uploads), c < C
static __global__ void __launch_bounds__(kBlock)
k_mge_init(CgState *__restrict__ st, int C)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    CgState s{};
    s.active = 1;
    st[c] = s;
}

// The report view: channel c's field k at data[c * stride_channel + k * stride_field]
struct MgeReport {
    double *data;
    long stride_channel, stride_field;
};

// Channel c's row of the report from st[c] and, in CCP_MG_NULLSPACE_CONSTANT mode, ns[c] (ns null: both means +0.0)
static __global__ void __launch_bounds__(kBlock)
k_mge_report(const CgState *__restrict__ st, const MgnState *__restrict__ ns, int C, MgeReport out)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    double *__restrict__ o = out.data + c * out.stride_channel;
    o[0] = (double)st[c].iterations;
    o[out.stride_field] = st[c].converged ? 1.0 : 0.0;
    o[2 * out.stride_field] = st[c].r1norm;
    o[3 * out.stride_field] = ns ? ns[c].b_mean : 0.0;
    o[4 * out.stride_field] = ns ? ns[c].x_mean : 0.0;
    o[5 * out.stride_field] = 0.0;
}

}  // namespace ccp
