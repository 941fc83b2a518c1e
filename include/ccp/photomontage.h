// ccp/photomontage.h — the image side of the path: drop-in counterparts of
// PhotoMontage::SolveChannel (project/src/PhotoMontage/PhotoMontage.cpp:535-628, same maths in
// labs/lab8/src/OpenCVHW1/hw8_pa.cc:902-986) and of the three-channel driver
// BuildSolveGradientFusion (PhotoMontage.cpp:410-436), on top of the C ABI (ccp_gs.h).
//
// OpenCV is not required: ccp::ImageView is a POD with cv::Mat's continuous row-major interleaved
// layout {data, rows, cols, channels, step}; `ccp::view(mat)` style adapters are one line
// (`ImageView{m.data, m.rows, m.cols, m.channels(), m.step}`).
//
// The solver is Gauss-Seidel (red-black, fixed iteration count — the slot where the reference
// calls conjugateGradient, PhotoMontage.cpp:613) or conjugate gradient; the matrix is never built.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccp_gs.h"

namespace ccp {

struct ImageView {
    void *data;
    int rows, cols, channels;
    std::size_t step;          // bytes per image row
};

// GaussSeidel: red-black order (the fast path).  GaussSeidelReferenceOrder: the reference's index-order
// sweep, iterates bit-identical to SparseMatrix::gaussSeidel on the matrix SolveChannel builds.
// MultigridConjugateGradient: CG preconditioned by a multigrid V-cycle (ccp_grid_mg_conjugate_gradient, 2 sweeps).
enum class Solver { GaussSeidel, ConjugateGradient, GaussSeidelReferenceOrder, MultigridConjugateGradient };

namespace detail {
inline void check(int status, const char *what)
{
    if (status != CCP_OK) throw std::runtime_error(std::string(what) + ": " + ccp_status_string(status));
}
struct GridHandle {
    ccp_grid *g = nullptr;
    GridHandle(int W, int H, int C, int device, int flags = 0)
    {
        ccp_grid_desc d{W, H, C, 0, H, 0, device, flags};
        check(ccp_grid_create(&d, &g), "ccp_grid_create");
    }
    ~GridHandle() { ccp_grid_destroy(g); }
    GridHandle(const GridHandle &) = delete;
    GridHandle &operator=(const GridHandle &) = delete;
};
inline void solve(ccp_grid *g, Solver solver, int iterations, int channels)
{
    std::vector<ccp_gs_report> rep(channels);
    if (solver == Solver::GaussSeidel)
        check(ccp_grid_gauss_seidel(g, 1e-10, iterations, /*check_every=*/0, rep.data()), "ccp_grid_gauss_seidel");
    else if (solver == Solver::GaussSeidelReferenceOrder)
        check(ccp_grid_gauss_seidel_lexicographic(g, 1e-10, iterations, /*check_every=*/0, rep.data()),
              "ccp_grid_gauss_seidel_lexicographic");
    else if (solver == Solver::MultigridConjugateGradient)
        check(ccp_grid_mg_conjugate_gradient(g, 1e-10, iterations, 2, rep.data()), "ccp_grid_mg_conjugate_gradient");
    else
        check(ccp_grid_conjugate_gradient(g, 1e-10, iterations, rep.data()), "ccp_grid_conjugate_gradient");
}
// the start vector without an `init`: 0 for the CG solvers (sparse-matrix.h:397), 1.0 for Gauss-Seidel (:352)
inline double default_start(Solver solver)
{
    return (solver == Solver::ConjugateGradient || solver == Solver::MultigridConjugateGradient) ? 0.0 : 1.0;
}
}  // namespace detail

// SolveChannel(channel_idx, constraint, color_gradient_x, color_gradient_y, output, ...)
// (PhotoMontage.h:24).  gx, gy: CV_32FC3 views (only y<H-1, x<W-1 are read), output: CV_8UC3 view
// whose channel `channel_idx` is written (clamped, PhotoMontage.cpp:617-626).  `init` (optional):
// CV_8UC3 composite image used as the start vector (fast_init_value, :599-610); without it Gauss-
// Seidel starts from 1.0 (sparse-matrix.h:352) and CG from 0 (:397), as the reference solvers do.
inline void SolveChannel(int channel_idx, int constraint, const ImageView &gx, const ImageView &gy, ImageView &output,
                         int iterations, const ImageView *init = nullptr, Solver solver = Solver::GaussSeidel,
                         int device = 0)
{
    const int W = gx.cols, H = gx.rows, C = gx.channels;
    if (gy.cols != W || gy.rows != H || gy.channels != C || output.cols != W || output.rows != H)
        throw std::invalid_argument("SolveChannel: image shapes differ");
    if (channel_idx < 0 || channel_idx >= C || channel_idx >= output.channels)
        throw std::invalid_argument("SolveChannel: bad channel index");
    // one-channel system: pick the channel's plane out of the interleaved gradients
    std::vector<float> px((std::size_t)W * H, 0.f), py((std::size_t)W * H, 0.f);
    for (int y = 0; y + 1 < H; ++y) {
        const float *rx = reinterpret_cast<const float *>(static_cast<const char *>(gx.data) + y * gx.step);
        const float *ry = reinterpret_cast<const float *>(static_cast<const char *>(gy.data) + y * gy.step);
        for (int x = 0; x + 1 < W; ++x) {
            px[(std::size_t)y * W + x] = rx[(std::size_t)x * C + channel_idx];
            py[(std::size_t)y * W + x] = ry[(std::size_t)x * C + channel_idx];
        }
    }
    detail::GridHandle h(W, H, 1, device);
    const int32_t pin = constraint;
    detail::check(ccp_grid_assemble_rhs(h.g, px.data(), py.data(), (int64_t)W * sizeof(float), &pin), "ccp_grid_assemble_rhs");
    if (init) {
        std::vector<uint8_t> plane((std::size_t)W * H);
        for (int y = 0; y < H; ++y) {
            const uint8_t *r = static_cast<const uint8_t *>(init->data) + y * init->step;
            for (int x = 0; x < W; ++x) plane[(std::size_t)y * W + x] = r[(std::size_t)x * init->channels + channel_idx];
        }
        detail::check(ccp_grid_set_x_u8(h.g, plane.data(), W), "ccp_grid_set_x_u8");
    } else {
        detail::check(ccp_grid_fill_x(h.g, detail::default_start(solver)), "ccp_grid_fill_x");
    }
    detail::solve(h.g, solver, iterations, 1);
    std::vector<uint8_t> out((std::size_t)W * H);
    detail::check(ccp_grid_store_u8(h.g, out.data(), W), "ccp_grid_store_u8");
    for (int y = 0; y < H; ++y) {
        uint8_t *r = static_cast<uint8_t *>(output.data) + y * output.step;
        for (int x = 0; x < W; ++x) r[(std::size_t)x * output.channels + channel_idx] = out[(std::size_t)y * W + x];
    }
}

// The reference's own member-function shape (PhotoMontage.h:24):
//     void SolveChannel(int channel_idx, int constraint, const cv::Mat &color_gradient_x, const cv::Mat &color_gradient_y,
//                       cv::Mat &output, const std::vector<cv::Mat> &Images);
// with the state it reads from its object (PhotoMontage.h:40,59; PhotoMontage.cpp:599-613): `iterations_`,
// `fast_init_value` and `result_label_` — when fast_init_value is set the start vector is the composite
// Images[result_label_(y, x)](y, x)[channel_idx].  A call site written against the reference class compiles against
// this one with cv::Mat replaced by ccp::ImageView; `solver` picks what runs in the slot of the reference's
// conjugateGradient call (:613).
class PhotoMontage {
public:
    int fast_init_value = 0;                 // PhotoMontage.h:40
    int iterations_ = 50;                    // PhotoMontage.h:59 (set by Run, PhotoMontage.cpp:248)
    ImageView result_label_{nullptr, 0, 0, 1, 0};   // CV_8UC1 (BuildSolveMRF's labelling; PhotoMontage.cpp:391)
    Solver solver = Solver::GaussSeidel;
    int device = 0;

    void SolveChannel(int channel_idx, int constraint, const ImageView &color_gradient_x, const ImageView &color_gradient_y,
                      ImageView &output, const std::vector<ImageView> &Images)
    {
        const int W = color_gradient_x.cols, H = color_gradient_x.rows;
        if (!fast_init_value) {
            ccp::SolveChannel(channel_idx, constraint, color_gradient_x, color_gradient_y, output, iterations_, nullptr, solver, device);
            return;
        }
        if (result_label_.data == nullptr || result_label_.cols != W || result_label_.rows != H)
            throw std::invalid_argument("PhotoMontage::SolveChannel: fast_init_value needs result_label_ of the gradients' shape");
        // the composite image (PhotoMontage.cpp:599-610): channel `channel_idx` of an interleaved image of the
        // gradients' channel count, which is the form the free function takes its start vector in
        const int C = color_gradient_x.channels;
        std::vector<uint8_t> comp((std::size_t)W * H * C, 0);
        for (int y = 0; y < H; ++y) {
            const uint8_t *lab = static_cast<const uint8_t *>(result_label_.data) + y * result_label_.step;
            for (int x = 0; x < W; ++x) {
                const std::size_t k = lab[(std::size_t)x * result_label_.channels];
                if (k >= Images.size()) throw std::invalid_argument("PhotoMontage::SolveChannel: label out of range");
                const ImageView &im = Images[k];
                if (im.cols != W || im.rows != H || channel_idx >= im.channels)
                    throw std::invalid_argument("PhotoMontage::SolveChannel: image shapes differ");
                comp[((std::size_t)y * W + x) * C + channel_idx] =
                    (static_cast<const uint8_t *>(im.data) + y * im.step)[(std::size_t)x * im.channels + channel_idx];
            }
        }
        const ImageView init{comp.data(), H, W, C, (std::size_t)W * C};
        ccp::SolveChannel(channel_idx, constraint, color_gradient_x, color_gradient_y, output, iterations_, &init, solver, device);
    }
};

// BuildSolveGradientFusion(Images, ResultLabel) (PhotoMontage.cpp:410-436): gradient field of the
// label-selected images, three channel solves, clamped CV_8UC3 result — all three channels in one
// device pass each.  images[k]: CV_8UC3 views of equal shape; label: CV_8UC1.
inline void BuildSolveGradientFusion(const std::vector<ImageView> &images, const ImageView &label, ImageView &result,
                                     int iterations, bool fast_init_value = true, Solver solver = Solver::GaussSeidel,
                                     int device = 0)
{
    if (images.empty()) throw std::invalid_argument("BuildSolveGradientFusion: no images");
    const int W = label.cols, H = label.rows;
    std::vector<const uint8_t *> ptrs;
    for (const auto &im : images) {
        if (im.cols != W || im.rows != H || im.channels != 3 || im.step != images[0].step)
            throw std::invalid_argument("BuildSolveGradientFusion: images must be CV_8UC3 of the label's shape");
        ptrs.push_back(static_cast<const uint8_t *>(im.data));
    }
    detail::GridHandle h(W, H, 3, device);
    detail::check(ccp_grid_assemble_from_images(h.g, ptrs.data(), (int32_t)ptrs.size(), (int64_t)images[0].step,
                                                static_cast<const uint8_t *>(label.data), (int64_t)label.step,
                                                fast_init_value ? 1 : 0),
                  "ccp_grid_assemble_from_images");
    if (!fast_init_value) detail::check(ccp_grid_fill_x(h.g, detail::default_start(solver)), "ccp_grid_fill_x");
    detail::solve(h.g, solver, iterations, 3);
    detail::check(ccp_grid_store_u8(h.g, static_cast<uint8_t *>(result.data), (int64_t)result.step), "ccp_grid_store_u8");
}

// ---- region blends: the system restricted to a pixel region (a Dirichlet-mask grid) -------------------------------
// mask: CV_8UC1 view, non-zero = region.  canvas / source / target / out: u8 views with the channel count of the
// blend, all of the mask's shape.  b and the start vector are built on the device, the solve is any Solver from the
// canvas (target) inside the region, and `out` receives the composite: the clamped solution inside the region, the
// canvas (target) outside.  Every failure throws; nothing is computed on the host.
enum class CloneMode { Import = CCP_CLONE_IMPORT, Mixed = CCP_CLONE_MIXED };

namespace detail {
inline void check_region_shape(const char *who, const ImageView &mask, std::initializer_list<const ImageView *> views, int C)
{
    if (mask.channels != 1 || !mask.data) throw std::invalid_argument(std::string(who) + ": mask must be a one-channel view");
    for (const ImageView *v : views)
        if (!v->data || v->rows != mask.rows || v->cols != mask.cols || v->channels != C)
            throw std::invalid_argument(std::string(who) + ": image shapes differ");
}
struct RegionHandle : GridHandle {
    RegionHandle(const ImageView &mask, int C, int device) : GridHandle(mask.cols, mask.rows, C, device, CCP_GRID_DIRICHLET_MASK)
    {
        check(ccp_grid_set_mask_host(g, static_cast<const uint8_t *>(mask.data), (int64_t)mask.step), "ccp_grid_set_mask_host");
    }
};
}  // namespace detail

// Region blend from a guidance field (lab8's union region, hw8_pa.cc:749-810): gx, gy float32 forward differences
// (CV_32FC<C> views sharing one row step), canvas u8: the Dirichlet values outside the region and the start vector.
inline void BlendRegion(const ImageView &gx, const ImageView &gy, const ImageView &canvas, const ImageView &mask,
                        ImageView &out, int iterations, Solver solver = Solver::GaussSeidel, int device = 0)
{
    const int C = canvas.channels;
    detail::check_region_shape("BlendRegion", mask, {&gx, &gy, &canvas, &out}, C);
    if (gx.step != gy.step) throw std::invalid_argument("BlendRegion: gx and gy must share one row step");
    detail::RegionHandle h(mask, C, device);
    detail::check(ccp_grid_assemble_region_rhs(h.g, static_cast<const float *>(gx.data), static_cast<const float *>(gy.data),
                                               (int64_t)gx.step, static_cast<const uint8_t *>(canvas.data), (int64_t)canvas.step, 1),
                  "ccp_grid_assemble_region_rhs");
    detail::solve(h.g, solver, iterations, C);
    detail::check(ccp_grid_store_u8_composite(h.g, static_cast<const uint8_t *>(canvas.data), (int64_t)canvas.step,
                                              static_cast<uint8_t *>(out.data), (int64_t)out.step),
                  "ccp_grid_store_u8_composite");
}

// Seamless cloning (Perez et al. 2003) of `source` into `target`, the source already placed on the canvas: imported
// or mixed gradients, boundary values and start vector from the target.  The region must not touch the canvas
// border (the call throws: CCP_ERR_UNSUPPORTED).
inline void SeamlessClone(const ImageView &source, const ImageView &target, const ImageView &mask, ImageView &out,
                          CloneMode mode, int iterations, Solver solver = Solver::GaussSeidel, int device = 0)
{
    const int C = target.channels;
    detail::check_region_shape("SeamlessClone", mask, {&source, &target, &out}, C);
    detail::RegionHandle h(mask, C, device);
    detail::check(ccp_grid_assemble_clone(h.g, static_cast<const uint8_t *>(source.data), (int64_t)source.step,
                                          static_cast<const uint8_t *>(target.data), (int64_t)target.step, (int32_t)mode, 1),
                  "ccp_grid_assemble_clone");
    detail::solve(h.g, solver, iterations, C);
    detail::check(ccp_grid_store_u8_composite(h.g, static_cast<const uint8_t *>(target.data), (int64_t)target.step,
                                              static_cast<uint8_t *>(out.data), (int64_t)out.step),
                  "ccp_grid_store_u8_composite");
}

// Weighted gradient-domain solve (CCP_GRID_WEIGHTED; screened Poisson fusion, WLS smoothing, soft constraints): for
// every channel, u minimises  sum wx (u(x+1,y) - u(x,y) - gx)^2 + sum wy (u(x,y+1) - u(x,y) - gy)^2 + sum lambda (u - f)^2.
// gx, gy, f: CV_32FC<C> views of out's shape (gx and gy sharing one row step), each may be null (zero); wx, wy, lambda:
// CV_32FC1 views sharing one row step, each may be null (wx, wy: 1 everywhere; lambda: 0).  The start vector is f (0
// without it); out: u8, the clamped solution.  Only Solver::MultigridConjugateGradient (at most `iterations` iterations,
// epsilon 1e-10) solves this system; any other solver throws std::invalid_argument, as does every other failure.
// hierarchy: the preconditioner's hierarchy kind (ccp_grid_mg_set_hierarchy); with lambda > 0 Hierarchy::Rescaled needs far
// fewer iterations, the default keeps the Galerkin one.
enum class Hierarchy { Galerkin = CCP_MG_HIERARCHY_GALERKIN, Rescaled = CCP_MG_HIERARCHY_RESCALED };
// precision: the preconditioner's precision (ccp_grid_mg_set_precision).  Precision::Single runs the V-cycle in float inside
// the fp64 loop: the same answer to the same epsilon; pair it with Hierarchy::Rescaled (with Hierarchy::Galerkin it costs
// iterations).  A weight too large or too small for a float makes the solve throw.  The default is the fp64 V-cycle.
enum class Precision { Double = CCP_MG_PRECISION_F64, Single = CCP_MG_PRECISION_F32 };
// channels: how the solve goes through the channels (ccp_grid_mg_set_channels).  Channels::Batched runs one PCG loop whose
// launches serve all channels; every channel gets the bits of the default, Channels::Sequential.  Not together with
// Precision::Single: that solve throws.
enum class Channels { Sequential = CCP_MG_CHANNELS_SEQUENTIAL, Batched = CCP_MG_CHANNELS_BATCHED };
// smoother: the V-cycle's smoother (ccp_grid_mg_set_smoother).  Smoother::Line is alternating zebra line relaxation, for
// strongly anisotropic weights (edge-aware smoothing, sparse fixed pixels); the default, Smoother::Point, is red-black
// Gauss-Seidel.  Not together with Precision::Single or Channels::Batched: that solve throws.
enum class Smoother { Point = CCP_MG_SMOOTHER_POINT, Line = CCP_MG_SMOOTHER_LINE };
// nullspace: the null space the solve accounts for (ccp_grid_mg_set_nullspace).  Nullspace::Constant solves the floating
// system -- lambda null or 0 everywhere, every in-canvas weight > 0: integrating a gradient field over the whole canvas --
// whose solution is free up to a constant per channel: the result keeps the mean of the start vector (f; 0 without it).
// Any other operator makes that solve throw, as does Channels::Batched.  The default, Nullspace::None, is the loop as it was.
enum class Nullspace { None = CCP_MG_NULLSPACE_NONE, Constant = CCP_MG_NULLSPACE_CONSTANT };

inline void SolveWeighted(const ImageView *gx, const ImageView *gy, const ImageView *f, const ImageView *wx, const ImageView *wy,
                          const ImageView *lambda, ImageView &out, int iterations,
                          Solver solver = Solver::MultigridConjugateGradient, int device = 0,
                          Hierarchy hierarchy = Hierarchy::Galerkin, Precision precision = Precision::Double,
                          Channels channels = Channels::Sequential, Smoother smoother = Smoother::Point,
                          Nullspace nullspace = Nullspace::None)
{
    if (solver != Solver::MultigridConjugateGradient)
        throw std::invalid_argument("SolveWeighted: only Solver::MultigridConjugateGradient solves a weighted system");
    const int C = out.channels;
    if (!out.data) throw std::invalid_argument("SolveWeighted: no output image");
    for (const ImageView *v : {gx, gy, f})
        if (v && (!v->data || v->rows != out.rows || v->cols != out.cols || v->channels != C))
            throw std::invalid_argument("SolveWeighted: image shapes differ");
    for (const ImageView *v : {wx, wy, lambda})
        if (v && (!v->data || v->rows != out.rows || v->cols != out.cols || v->channels != 1))
            throw std::invalid_argument("SolveWeighted: weights must be one-channel views of the image's shape");
    if (gx && gy && gx->step != gy->step) throw std::invalid_argument("SolveWeighted: gx and gy must share one row step");
    std::size_t wstep = 0;
    for (const ImageView *v : {wx, wy, lambda})
        if (v) {
            if (wstep && v->step != wstep) throw std::invalid_argument("SolveWeighted: the weights must share one row step");
            wstep = v->step;
        }
    auto fp = [](const ImageView *v) { return v ? static_cast<const float *>(v->data) : nullptr; };
    detail::GridHandle h(out.cols, out.rows, C, device, CCP_GRID_WEIGHTED);
    detail::check(ccp_grid_mg_set_hierarchy(h.g, (int32_t)hierarchy), "ccp_grid_mg_set_hierarchy");
    detail::check(ccp_grid_mg_set_precision(h.g, (int32_t)precision), "ccp_grid_mg_set_precision");
    detail::check(ccp_grid_mg_set_channels(h.g, (int32_t)channels), "ccp_grid_mg_set_channels");
    detail::check(ccp_grid_mg_set_smoother(h.g, (int32_t)smoother), "ccp_grid_mg_set_smoother");
    detail::check(ccp_grid_mg_set_nullspace(h.g, (int32_t)nullspace), "ccp_grid_mg_set_nullspace");
    detail::check(ccp_grid_set_weights_host(h.g, fp(wx), fp(wy), fp(lambda), (int64_t)wstep), "ccp_grid_set_weights_host");
    const int64_t gstep = gx ? (int64_t)gx->step : gy ? (int64_t)gy->step : 0;
    detail::check(ccp_grid_assemble_weighted_rhs(h.g, fp(gx), fp(gy), gstep, fp(f), f ? (int64_t)f->step : 0, f ? 1 : 0),
                  "ccp_grid_assemble_weighted_rhs");
    if (!f) detail::check(ccp_grid_fill_x(h.g, 0.0), "ccp_grid_fill_x");
    detail::solve(h.g, solver, iterations, C);
    detail::check(ccp_grid_store_u8(h.g, static_cast<uint8_t *>(out.data), (int64_t)out.step), "ccp_grid_store_u8");
}

// SolveWeighted with hard constraints (include/ccp_gs.h, "Hard constraints on weighted grids"): the pixels where `fixed`
// (a one-channel u8 view, non-zero = fixed) is set keep the value `values` prescribes (float32, the image's shape; NULL:
// 0), and the energy is minimised over the others from the start vector f (0 without f).  The free region may touch the
// canvas border.  out: the clamped composite, the solution on the free pixels and `values` on the fixed ones.  With
// lambda NULL or 0 every connected set of free pixels needs a fixed neighbour.
inline void SolveConstrained(const ImageView *gx, const ImageView *gy, const ImageView *f, const ImageView *values, const ImageView &fixed,
                             const ImageView *wx, const ImageView *wy, const ImageView *lambda, ImageView &out, int iterations,
                             int device = 0, Hierarchy hierarchy = Hierarchy::Rescaled, Precision precision = Precision::Double,
                             Channels channels = Channels::Sequential, Smoother smoother = Smoother::Point)
{
    const int C = out.channels;
    if (!out.data) throw std::invalid_argument("SolveConstrained: no output image");
    for (const ImageView *v : {gx, gy, f, values})
        if (v && (!v->data || v->rows != out.rows || v->cols != out.cols || v->channels != C))
            throw std::invalid_argument("SolveConstrained: image shapes differ");
    for (const ImageView *v : {wx, wy, lambda, &fixed})
        if (v && (!v->data || v->rows != out.rows || v->cols != out.cols || v->channels != 1))
            throw std::invalid_argument("SolveConstrained: weights and mask must be one-channel views of the image's shape");
    if (gx && gy && gx->step != gy->step) throw std::invalid_argument("SolveConstrained: gx and gy must share one row step");
    std::size_t wstep = 0;
    for (const ImageView *v : {wx, wy, lambda})
        if (v) {
            if (wstep && v->step != wstep) throw std::invalid_argument("SolveConstrained: the weights must share one row step");
            wstep = v->step;
        }
    auto fp = [](const ImageView *v) { return v ? static_cast<const float *>(v->data) : nullptr; };
    detail::GridHandle h(out.cols, out.rows, C, device, CCP_GRID_WEIGHTED);
    detail::check(ccp_grid_mg_set_hierarchy(h.g, (int32_t)hierarchy), "ccp_grid_mg_set_hierarchy");
    detail::check(ccp_grid_mg_set_precision(h.g, (int32_t)precision), "ccp_grid_mg_set_precision");
    detail::check(ccp_grid_mg_set_channels(h.g, (int32_t)channels), "ccp_grid_mg_set_channels");
    detail::check(ccp_grid_mg_set_smoother(h.g, (int32_t)smoother), "ccp_grid_mg_set_smoother");
    detail::check(ccp_grid_set_weights_constrained_host(h.g, fp(wx), fp(wy), fp(lambda), (int64_t)wstep,
                                                        static_cast<const uint8_t *>(fixed.data), (int64_t)fixed.step),
                  "ccp_grid_set_weights_constrained_host");
    if (!f) detail::check(ccp_grid_fill_x(h.g, 0.0), "ccp_grid_fill_x");
    const int64_t gstep = gx ? (int64_t)gx->step : gy ? (int64_t)gy->step : 0;
    detail::check(ccp_grid_assemble_constrained_rhs(h.g, fp(gx), fp(gy), gstep, fp(f), f ? (int64_t)f->step : 0, fp(values),
                                                    values ? (int64_t)values->step : 0, f ? 1 : 0),
                  "ccp_grid_assemble_constrained_rhs");
    detail::solve(h.g, Solver::MultigridConjugateGradient, iterations, C);
    detail::check(ccp_grid_store_u8(h.g, static_cast<uint8_t *>(out.data), (int64_t)out.step), "ccp_grid_store_u8");
}

}  // namespace ccp
