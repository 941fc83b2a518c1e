// ccp_grid_weighted.hip — the weighted handle's operator kernels (ccp_grid_weighted.hpp) and the per-channel batched
// mode's (ccp_grid_pco.hpp) in a translation unit of their own, behind the launchers ccp_grid.hip and ccp_grid_mg.hip call.
#include "ccp_grid_pco.hpp"
#include "ccp_grid_weighted.hpp"

#include <atomic>

using namespace ccp;

namespace {

dim3 pixels(int W, int H, int C) { return dim3((unsigned)((W + kBlock - 1) / kBlock), (unsigned)H, (unsigned)C); }

}  // namespace

int ccp::weighted_coef(hipStream_t s, const ImageView &wx, const ImageView &wy, const ImageView &lam, const ImageView *fixed, int W, int H,
                       int sets, long pitch, double *op, long plane, double *cons, unsigned long long *count)
{
    CCP_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long) * (size_t)(1 + 3 * sets), s));
    if (fixed)
        hipLaunchKernelGGL(k_weighted_coef_fixed, pixels(W, H, sets), dim3(kBlock), 0, s, wx, wy, lam, *fixed, W, H, pitch, op, plane, 4 * plane,
                           cons, 3 * plane, count);
    else
        hipLaunchKernelGGL(k_weighted_coef, pixels(W, H, sets), dim3(kBlock), 0, s, wx, wy, lam, W, H, pitch, op, plane, 4 * plane, count);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::weighted_rhs(hipStream_t s, double *b, double *x, const Geom &g, int C, int sets, const double *op, const double *cons,
                      const ImageView &gx, const ImageView &gy, const ImageView &f, const ImageView &v, int has, bool init)
{
    const long plane = g.ch_stride;
    const dim3 grid = pixels(g.W, g.H, sets);
    with_bool(init, [&](auto I) {
        with_bool(cons != nullptr, [&](auto F) {
            hipLaunchKernelGGL((k_weighted_rhs<decltype(I)::value, decltype(F)::value>), grid, dim3(kBlock), 0, s, b, x, g, op, plane, 4 * plane,
                               cons, 3 * plane, gx, gy, f, v, cons ? has : has & 7, C / sets);
        });
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::weighted_coarsen(hipStream_t s, int sets, const MgLevel &lv, long fs, const double *lam, long ls, const MgLevel &cv, double *d,
                          double *we, double *ws, double *lam_c, long cstride, double edge)
{
    hipLaunchKernelGGL(k_weighted_coarsen, pixels(cv.W, cv.H, sets), dim3(kBlock), 0, s, lv, fs, lam, ls, cv, d, we, ws, lam_c, cstride, edge);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

// k_pco_tile's five planes pass the 64 KiB a kernel may take without asking (115,200 B at nu = 2): once per device and process
int ccp::pco_tile_lds_limit()
{
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    CCP_HIP(hipGetDevice(&dev));
    const unsigned long long bit = dev < 64 ? 1ull << dev : 0;
    if (raised.load() & bit) return CCP_OK;
    const int bytes = mgb_tile_lds(kMgCoarse, 4);                    // the largest nu
    CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pco_tile<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    CCP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pco_tile<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    raised.fetch_or(bit);
    return CCP_OK;
}

int ccp::pco_tile(hipStream_t s, bool post, dim3 tiles, int C, const MgLevel &lv, long os, const double *b, const double *z_in, double *z_out,
                  long fs, const MgLevel &cv, const double *ec, long es, double cs, int nu, const CgState *st)
{
    tiles.z = (unsigned)C;
    with_bool(post, [&](auto P) {
        hipLaunchKernelGGL((k_pco_tile<decltype(P)::value>), tiles, dim3(mgb_tile_threads(kMgCoarse)), mgb_tile_lds(kMgCoarse, nu), s, lv, os, b,
                           z_in, z_out, fs, cv, ec, es, cs, nu, st);
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_restrict(hipStream_t s, int C, const MgLevel &lv, long os, const double *b, const double *z, long fs, const MgLevel &cv, double *bc,
                      long es, const CgState *st)
{
    hipLaunchKernelGGL(k_pco_restrict, pixels(cv.W, cv.H, C), dim3(kBlock), 0, s, lv, os, b, z, fs, cv, bc, es, st);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_tail(hipStream_t s, int C, const MgTail *tails, const double *b_top, double *z_top, long bs, long zs, double cs, int nu,
                  const CgState *st)
{
    hipLaunchKernelGGL(k_pco_tail, dim3((unsigned)C), dim3(kBlock), 0, s, tails, b_top, z_top, bs, zs, cs, nu, st);
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

int ccp::pco_apply(hipStream_t s, bool dot, dim3 grid, int C, const MgLevel &lv, long os, const double *in, double *out, long vs,
                   double *partial, long ps, const CgState *st)
{
    grid.z = 2 * (unsigned)C;
    with_bool(dot, [&](auto D) {
        hipLaunchKernelGGL((k_pco_apply<decltype(D)::value>), grid, dim3(kBlock), 0, s, lv, os, in, out, vs, partial, ps, st);
    });
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}
