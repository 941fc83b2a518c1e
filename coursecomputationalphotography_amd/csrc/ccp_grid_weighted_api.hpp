// ccp_grid_weighted_api.hpp — what ccp_grid_mg.hip needs of the weighted handle's coarsening kernel
// (ccp_grid_weighted.hpp) and of the per-channel batched mode's kernels (ccp_grid_pco.hpp), all compiled in
// ccp_grid_weighted.hip alone: the launchers; and, the other way, what ccp_grid_weighted.hip's refresh entry point needs of
// the hierarchy.  No kernels here, so that including it adds nothing to a
// translation unit's device code.
#pragma once

#include "ccp_common.hpp"

namespace ccp {

struct MgLevel;
struct CgState;
template <typename T>
struct MgTailT;

// ---- the launchers (ccp_grid_weighted.hip); each enqueues one launch on `s` and returns the launch's status ------------

// one level of `sets` hierarchies in one launch
int weighted_coarsen(hipStream_t s, int sets, const MgLevel &lv, long fs, const double *lam, long ls, const MgLevel &cv, double *d, double *we,
                     double *ws, double *lam_c, long cstride, double edge);

// one operator per channel, the batched mode's passes: `os` the per-channel stride of lv's coefficients, the other arguments as the kernels'
int pco_tile_lds_limit();                                            // once per device: k_pco_tile may take mgb_tile_lds(kMgCoarse, 4)
int pco_tile(hipStream_t s, bool post, dim3 tiles, int C, const MgLevel &lv, long os, const double *b, const double *z_in, double *z_out, long fs,
             const MgLevel &cv, const double *ec, long es, double cs, int nu, const CgState *st);
int pco_restrict(hipStream_t s, int C, const MgLevel &lv, long os, const double *b, const double *z, long fs, const MgLevel &cv, double *bc,
                 long es, const CgState *st);
int pco_tail(hipStream_t s, int C, const MgTailT<double> *tails, const double *b_top, double *z_top, long bs, long zs, double cs, int nu,
             const CgState *st);
int pco_apply(hipStream_t s, bool dot, dim3 grid, int C, const MgLevel &lv, long os, const double *in, double *out, long vs, double *partial,
              long ps, const CgState *st);

// ---- the other way (ccp_grid_mg.hip): the hierarchy's half of ccp_grid_refresh_weights_device --------------------------
// CCP_ERR_STATE with nothing enqueued unless ccp_grid_mg_prepare's work stands; else one launch: the status word, n_counts
// words of the refresh pass's counts and the mode's verdict words zeroed
int mg_refresh_begin(ccp_grid *g, int n_counts);
// the same question alone, nothing enqueued: CCP_OK while ccp_grid_mg_prepare's work stands (b and x are the enqueue solve's)
int mg_prepared(ccp_grid *g);
int mg_refresh(ccp_grid *g);         // the coarse levels, float copies, census and status word from the new level 0: launches only

}  // namespace ccp
