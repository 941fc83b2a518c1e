// ccp_grid_mge.hpp — the kernels of the enqueue-only multigrid PCG (include/ccp_gs.h:
// ccp_grid_mg_conjugate_gradient_enqueue) and the status fold of ccp_grid_refresh_weights_device, hand-written for gfx950.  The recurrence, its kernels and its launch geometry
// are the synchronous call's (ccp_grid_mg.hpp, ccp_cg.hpp, ccp_grid_mgn.hpp); what the host does there with copies is done
// here on the device:
//
//   k_mge_init     the C CgStates of a solve, where the synchronous call uploads them from the host
//   k_mge_report   the report of C channels into a strided view of device memory, where the synchronous call reads the
//                  states back and fills ccp_gs_report
//
//   k_mge_clear    the words the refresh's kernels OR and count into, zeroed
//   k_mge_status   the verdicts of a refreshed operator into one device word, where the setters and ccp_grid_mg_prepare
//                  read theirs back
//
// Each is one workgroup of plain vector stores, one lane per channel (C <= kMaxChannels) or one lane in all.
#pragma once

#include "ccp_grid_mgn.hpp"

namespace ccp {

constexpr int kMgeReportFields = 6;   // iterations, converged, last_l1_step, b_mean, x_mean, reserved

// st[c] := a state about to start (active, every count and scalar 0: what pcg_loop uploads), c < C.  status: the
// operator status word of ccp_grid_refresh_weights_device (0 while a setter's operator is installed), or null on a handle
// that is not weighted; while it is non-zero every channel starts stopped (active 0), so every later launch of the solve
// is a no-op.
static __global__ void __launch_bounds__(kBlock)
k_mge_init(CgState *__restrict__ st, int C, const unsigned *__restrict__ status)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    CgState s{};
    s.active = status && *status ? 0 : 1;
    st[c] = s;
}

// The first launch of ccp_grid_refresh_weights_device: the status word, the refresh pass's verdict and counts (n_counts
// words, <= kBlock) and, where the mode has them (null otherwise), the narrowing's flag and the census counts
// (kMaxChannels words) := 0.  A kernel and not hipMemsetAsync: the refresh is made to be captured, and the memset nodes
// of a captured graph did not clear these words on replay (NOTES.md R32.2).
static __global__ void __launch_bounds__(kBlock)
k_mge_clear(unsigned *__restrict__ status, unsigned long long *__restrict__ counts, int n_counts, unsigned *__restrict__ fbad,
            unsigned *__restrict__ census)
{
    const int t = threadIdx.x;
    if (t == 0) *status = 0;
    if (t < n_counts) counts[t] = 0;
    if (fbad && t == 0) *fbad = 0;
    if (census && t < kMaxChannels) census[t] = 0;
}

// The last launch of ccp_grid_refresh_weights_device: the three verdicts of the refreshed operators ORed into the status
// word (include/ccp_gs.h, CCP_OPERATOR_*), which k_mge_clear cleared.  verdict[0] != 0: a weight
// failed k_weighted_refresh's check; fbad (null unless CCP_MG_PRECISION_F32): k_mgs_narrow's flag; census (null unless
// CCP_MG_NULLSPACE_CONSTANT): k_mgn_census's count of every one of the `sets` operators.
static __global__ void __launch_bounds__(kBlock)
k_mge_status(const unsigned long long *__restrict__ verdict, const unsigned *__restrict__ fbad, const unsigned *__restrict__ census, int sets,
             unsigned *__restrict__ status)
{
    if (threadIdx.x != 0) return;
    unsigned w = *status;
    if (verdict[0]) w |= 1u;
    if (fbad && *fbad) w |= 2u;
    for (int k = 0; census && k < sets; ++k)
        if (census[k]) w |= 4u;
    *status = w;
}

// The report view: channel c's field k at data[c * stride_channel + k * stride_field]
struct MgeReport {
    double *data;
    long stride_channel, stride_field;
};

// Channel c's row of the report from st[c] and, in CCP_MG_NULLSPACE_CONSTANT mode, ns[c] (ns null: both means +0.0);
// field [5]: the operator status word as a double (status null: +0.0)
static __global__ void __launch_bounds__(kBlock)
k_mge_report(const CgState *__restrict__ st, const MgnState *__restrict__ ns, int C, MgeReport out, const unsigned *__restrict__ status)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    double *__restrict__ o = out.data + c * out.stride_channel;
    o[0] = (double)st[c].iterations;
    o[out.stride_field] = st[c].converged ? 1.0 : 0.0;
    o[2 * out.stride_field] = st[c].r1norm;
    o[3 * out.stride_field] = ns ? ns[c].b_mean : 0.0;
    o[4 * out.stride_field] = ns ? ns[c].x_mean : 0.0;
    o[5 * out.stride_field] = status ? (double)*status : 0.0;
}

}  // namespace ccp
