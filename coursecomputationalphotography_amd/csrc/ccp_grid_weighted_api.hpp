// ccp_grid_weighted_api.hpp — what ccp_grid.hip and ccp_grid_mg.hip need of the weighted handle's operator kernels
// (ccp_grid_weighted.hpp) and of the per-channel batched mode's (ccp_grid_pco.hpp), all compiled in
// ccp_grid_weighted.hip alone: the launchers.  No kernels here, so that including it adds nothing to a
// translation unit's device code.
#pragma once

#include "ccp_common.hpp"
#include "ccp_grid_geom.hpp"
#include "ccp_view.hpp"

namespace ccp {

struct MgLevel;
struct CgState;
template <typename T>
struct MgTailT;

// ---- the launchers (ccp_grid_weighted.hip); each enqueues one launch on `s` and returns the launch's status ------------

// The planes of `sets` operators (1: the one all channels share, from H x W views; C: one per channel) in one launch;
// fixed: null for none (cons is not touched then).  count: 1 + 3 sets words, zeroed here.
int weighted_coef(hipStream_t s, const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView *fixed, int W, int H, int sets,
                  long pitch, double *op, long plane, double *cons, unsigned long long *count);
// b (and x at fixed pixels, or everywhere with init) of all C channels from `sets` operators in one launch; cons: null
// without fixed pixels
int weighted_rhs(hipStream_t s, double *b, double *x, const Geom &g, int C, int sets, const double *op, const double *cons,
                 const ImageView &gx, const ImageView &gy, const ImageView &f, const ImageView &v, int has, bool init);
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

}  // namespace ccp
