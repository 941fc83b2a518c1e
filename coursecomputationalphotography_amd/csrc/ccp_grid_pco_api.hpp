// ccp_grid_pco_api.hpp — what ccp_grid.hip and ccp_grid_mg.hip need of the per-channel operator's kernels
// (ccp_grid_pco.hpp, compiled in ccp_grid_pco.hip alone): the view type and the launchers.  No kernels here, so that
// including it adds nothing to a translation unit's device code.
#pragma once

#include "ccp_common.hpp"
#include "ccp_grid_geom.hpp"

namespace ccp {

struct MgLevel;
struct CgState;
template <typename T>
struct MgTailT;

// An H x W x C array of the per-channel calls: u8, f32 or f64 elements `sy`, `sx`, `sc` apart (0 broadcasts), or none
// (p == nullptr): `dflt` everywhere.  The dtype is uniform over a launch, so the branch costs no divergence; every
// conversion to double is exact.
struct PcoView {
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
};

// ---- the launchers (ccp_grid_pco.hip); each enqueues one launch on `s` and returns the launch's status -----------------

// All channels' planes in one launch; fixed: null for none (cons is not touched then).  count: 1 + 3 C words, zeroed here.
int pco_coef(hipStream_t s, const PcoView &wx, const PcoView &wy, const PcoView &lam, const PcoView *fixed, int W, int H, int C, long pitch,
             double *op, long plane, double *cons, unsigned long long *count);
// b (and x at fixed pixels, or everywhere with init) of all channels in one launch; cons: null without fixed pixels
int pco_rhs(hipStream_t s, double *b, double *x, const Geom &g, int C, const double *op, const double *cons, const PcoView &gx,
            const PcoView &gy, const PcoView &f, const PcoView &v, int has, bool init);
// one level of all channels' hierarchies in one launch
int pco_coarsen(hipStream_t s, int C, const MgLevel &lv, long fs, const double *lam, long ls, const MgLevel &cv, double *d, double *we,
                double *ws, double *lam_c, long cstride, double edge);

// the batched mode's passes: `os` the per-channel stride of lv's coefficients, the other arguments as the kernels'
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
