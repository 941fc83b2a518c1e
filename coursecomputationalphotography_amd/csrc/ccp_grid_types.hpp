// ccp_grid_types.hpp — the plain types and constants a grid handle (ccp_grid_handle.hpp) holds that belong to kernel
// headers: no kernels here, so that the handle can be seen by a translation unit that does not compile those kernels.
#pragma once

#include "ccp_common.hpp"

namespace ccp {

// ---- ccp_grid_fused.hpp --------------------------------------------------------------------------------------------------
#ifndef CCP_FUSED_MAX_T
#define CCP_FUSED_MAX_T 8
#endif
constexpr int kFusedMaxT = CCP_FUSED_MAX_T;          // deepest pass instantiated
constexpr int kFusedMaxCheckedT = 8;     // deepest pass that also reports the step of each of its sweeps (+2T+4 VGPRs)

// ---- ccp_grid_kernels.hpp ------------------------------------------------------------------------------------------------
// Per-channel solver state kept on the device so the stop rule needs no host round trip.
struct SolveState {
    int active[kMaxChannels];       // 1 while the channel still iterates
    int converged[kMaxChannels];
    int iterations[kMaxChannels];   // sweep index at which the stop rule fired
    double last_eps[kMaxChannels];
};

// ---- ccp_grid_lex.hpp ----------------------------------------------------------------------------------------------------
struct LexGeom {
    int W, H;
    long P;          // doubles per diagonal row (>= W)
    long plane;      // doubles per channel = (W+H-1) * P
    int n_diag;      // W + H - 1
    int nbx;         // blocks along the longest diagonal
};

}  // namespace ccp
