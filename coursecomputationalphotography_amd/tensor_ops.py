"""Poisson solves on torch tensors: the tensor counterparts of the C++ facade's ccp::SolveChannel, ccp::BlendRegion
and ccp::SeamlessClone (include/ccp/photomontage.h), on the device hand-off of a grid handle (Grid.*_tensor).

Images stay on the GPU from input to result: the right-hand side is assembled from the tensors on the device, the
solve runs there, and the result is a u8 tensor on the same device.  Every call is enqueued on torch's current stream
of that device; the solvers themselves wait for their own reports, so the call returns once the solve is done.
`solver` takes the names of the facade's ccp::Solver: "GaussSeidel" (red-black), "ConjugateGradient",
"GaussSeidelReferenceOrder" and "MultigridConjugateGradient"; `iterations` means what it means there (fixed sweep
count for the Gauss-Seidel solvers, the iteration cap at epsilon 1e-10 for the CG solvers).
WeightedSolver is the exception to "the solvers wait": a persistent weighted handle whose solves only enqueue.
"""
from __future__ import annotations

import numpy as np

from . import capi

SOLVERS = ("GaussSeidel", "ConjugateGradient", "GaussSeidelReferenceOrder", "MultigridConjugateGradient")


def _solve(g: "capi.Grid", solver: str, iterations: int) -> None:
    if solver == "GaussSeidel":
        g.gauss_seidel(1e-10, iterations, check_every=0)
    elif solver == "GaussSeidelReferenceOrder":
        g.gauss_seidel_lexicographic(1e-10, iterations, check_every=0)
    elif solver == "MultigridConjugateGradient":
        g.mg_conjugate_gradient(1e-10, iterations, 2)
    else:
        g.conjugate_gradient(1e-10, iterations)


def _check_solver(solver: str) -> None:
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, not {solver!r}")


def _device_index(t) -> int:
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError("inputs must be torch tensors on a GPU")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _grid(W, H, C, dev, mask=None) -> "capi.Grid":
    """A handle whose every call, the solve included, is enqueued on torch's current stream of `dev`."""
    import torch
    if isinstance(mask, torch.Tensor) and mask.device.type == "cuda":
        if mask.dtype not in (torch.bool, torch.uint8, torch.float32, torch.float64):
            mask = mask != 0
        mask = mask.to(torch.device("cuda", dev))                 # (a mask on another GPU: one device-to-device copy)
    elif mask is not None:
        mask = _host_mask(mask)
    g = capi.Grid(W, H, C, device=dev, mask=mask)
    g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
    return g


def _host_mask(mask) -> np.ndarray:
    """A numpy or CPU-tensor mask as a host array (a CUDA tensor goes to the handle as it is: Grid.set_mask_tensor)."""
    import torch
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    return np.asarray(mask)


def solve_channels(gx, gy, constraint, iterations: int, init=None, solver: str = "GaussSeidel", precision="f64",
                   channels="sequential"):
    """Every channel of SolveChannel's system at once: b from float32 H x W x C gradient tensors and the pin values
    `constraint` (one int per channel), the start vector from the u8 H x W x C tensor `init` (the composite of
    fast_init_value) or, without it, 1.0 for Gauss-Seidel and 0 for CG, as the reference solvers start.  Returns the
    clamped solution as a u8 H x W x C tensor.  precision: "f64" or "f32", the V-cycle's precision when the solver is
    "MultigridConjugateGradient" (capi.Grid.mg_set_precision); the other solvers take "f64" only.  channels: "sequential" or "batched"
    (capi.Grid.mg_set_channels: one PCG loop for all channels, the same bits), likewise for that solver only."""
    _check_solver(solver)
    if channels != "sequential" and solver != "MultigridConjugateGradient":
        raise ValueError("channels applies to solver 'MultigridConjugateGradient' only")
    if precision != "f64" and solver != "MultigridConjugateGradient":
        raise ValueError("precision applies to solver 'MultigridConjugateGradient' only")
    dev = _device_index(gx)
    H, W = gx.shape[0], gx.shape[1]
    C = gx.shape[2] if gx.dim() == 3 else 1
    g = _grid(W, H, C, dev)
    try:
        g.mg_configure(precision=precision, channels=channels)
        g.assemble_rhs_tensor(gx, gy, constraint)
        if init is not None:
            g.set_x_u8_tensor(init)
        else:
            g.fill_x(0.0 if solver in ("ConjugateGradient", "MultigridConjugateGradient") else 1.0)
        _solve(g, solver, iterations)
        return g.store_u8_tensor()
    finally:
        g.close()


def blend_region(gx, gy, canvas, mask, iterations: int, solver: str = "GaussSeidel"):
    """Region blend from a guidance field (ccp::BlendRegion): gx, gy float32 H x W x C tensors, canvas u8 H x W x C
    (the values outside the region and the start vector), mask H x W (non-zero = region).  Returns the composite,
    a u8 H x W x C tensor.  A CUDA mask tensor is read on the device (capi.Grid.set_mask_tensor); a numpy or CPU
    mask goes through the host setter."""
    _check_solver(solver)
    dev = _device_index(canvas)
    H, W = canvas.shape[0], canvas.shape[1]
    C = canvas.shape[2] if canvas.dim() == 3 else 1
    g = _grid(W, H, C, dev, mask)
    try:
        g.assemble_region_rhs_tensor(gx, gy, canvas, init_x=True)
        _solve(g, solver, iterations)
        return g.store_u8_composite_tensor(canvas)
    finally:
        g.close()


def seamless_clone(source, target, mask, iterations: int, mixed: bool = False, solver: str = "GaussSeidel"):
    """Seamless cloning (ccp::SeamlessClone) of the u8 H x W x C tensor `source`, already placed on the canvas, into
    `target`: imported (mixed False) or mixed gradients, boundary values and start vector from the target.  mask
    H x W (see blend_region); a region touching the canvas border raises CcpError.  Returns
    the composite, a u8 H x W x C tensor."""
    _check_solver(solver)
    dev = _device_index(target)
    H, W = target.shape[0], target.shape[1]
    C = target.shape[2] if target.dim() == 3 else 1
    g = _grid(W, H, C, dev, mask)
    try:
        g.assemble_clone_tensor(source, target, mixed=mixed, init=1)
        _solve(g, solver, iterations)
        return g.store_u8_composite_tensor(target)
    finally:
        g.close()


def panorama_merge(images, footprints):
    """lab8's merge (hw8_pa.cc:749-799) of u8 H x W x C image tensors already warped onto one canvas, with their u8
    H x W footprint masks: the first image starts the state, every further one is merged in under its footprint eroded
    2 (outer) and 4 (inner) times with the 3 x 3 cross (:718-722), and the gradients along the rim of the union are
    recomputed from the merged colours.  Returns (dx, dy, raw, mask): float32, float32, u8 H x W x C and u8 H x W
    tensors, bit for bit what lab8_workload's numpy restatement computes.  Nothing leaves the device."""
    if len(images) < 1 or len(images) != len(footprints):
        raise ValueError("one footprint per image, at least one image")
    state = capi.panorama_begin_tensor(images[0], footprints[0])
    for img, foot in zip(images[1:], footprints[1:]):
        capi.panorama_add_tensor(state, img, capi.mask_erode_cross_tensor(foot, 2), capi.mask_erode_cross_tensor(foot, 4))
    capi.panorama_finish_tensor(state)
    return state


def panorama_blend(images, footprints, iterations: int = 50, solver: str = "GaussSeidel"):
    """lab8's panorama blend from device tensors to a device result: panorama_merge, then the Poisson system of the
    merged field on the union mask with the merged colours as boundary values and start vector (hw8_pa.cc:808-810,
    50 iterations there), solved by `solver`; returns the composite, a u8 H x W x C tensor.  No image or mask is
    copied to the host."""
    _check_solver(solver)
    dx, dy, raw, mask = panorama_merge(images, footprints)
    dev = _device_index(raw)
    H, W = raw.shape[0], raw.shape[1]
    C = raw.shape[2] if raw.dim() == 3 else 1
    g = _grid(W, H, C, dev, mask)
    try:
        g.assemble_region_rhs_tensor(dx, dy, raw, init_x=True)
        _solve(g, solver, iterations)
        return g.store_u8_composite_tensor(raw)
    finally:
        g.close()


def _weight(w, H, W, dev):
    """A weight argument of weighted_solve: None stays None (the library's default), a scalar becomes a broadcast
    H x W float64 view (stride 0: nothing is materialised), a tensor is passed as it is."""
    import torch
    if w is None or isinstance(w, torch.Tensor):
        return w
    return torch.tensor(float(w), dtype=torch.float64, device=torch.device("cuda", dev)).expand(H, W)


def _per_channel(*tensors):
    """Does any of the operator's arguments carry a channel axis (H x W x C)?  Then the handle gets one operator per
    channel (capi.Grid.set_weights_per_channel_tensor); otherwise exactly the shared operator's path."""
    import torch
    return any(isinstance(t, torch.Tensor) and t.dim() == 3 for t in tensors)


def _set_operator(g, wx, wy, lam, fixed=None):
    if _per_channel(wx, wy, lam, fixed):
        g.set_weights_per_channel_tensor(wx, wy, lam, fixed)
    else:
        g.set_weights_tensor(wx, wy, lam, fixed=fixed)


def weighted_solve(gx, gy, f, iterations: int, wx=None, wy=None, data_weight=None, out_dtype=None, epsilon: float = 1e-10,
                   hierarchy="galerkin", precision="f64", channels="sequential", smoother="point", nullspace="none"):
    """Minimise  sum wx (u(x+1,y) - u(x,y) - gx)^2 + sum wy (u(x,y+1) - u(x,y) - gy)^2 + sum data_weight (u - f)^2
    for every channel on a weighted grid handle (CCP_GRID_WEIGHTED), by multigrid-preconditioned CG (at most
    `iterations` iterations to sqrt(r'r) < epsilon) from x = f.  gx, gy: float32 H x W x C tensors or None (zero
    guidance); f: u8 / float32 / float64 H x W x C or None (zero, and x starts at 0).  wx, wy, data_weight: H x W
    float32 / float64 tensors or scalars (None: wx = wy = 1, data_weight = 0).  out_dtype: torch.uint8 (the default: the
    clamped solution) or a float dtype (x itself).  hierarchy: "galerkin" (the default) or "rescaled"
    (capi.Grid.mg_set_hierarchy): with data_weight > 0 "rescaled" needs far fewer iterations.  precision: "f64" (the
    default) or "f32" (capi.Grid.mg_set_precision: the V-cycle in float inside the fp64 loop, the same answer to the same
    epsilon; choose it together with "rescaled", the Galerkin hierarchy pays iterations for it).  channels: "sequential" (the
    default) or "batched" (capi.Grid.mg_set_channels: one PCG loop whose launches serve all channels; every channel gets
    the same bits; not together with "f32").  smoother: "point" (the default) or "line" (capi.Grid.mg_set_smoother:
    alternating zebra line relaxation, for strongly anisotropic weights; fp64 and sequential channels only).
    nullspace: "none" (the default) or "constant" (capi.Grid.mg_set_nullspace): the floating system -- data_weight None or
    0 everywhere and every in-canvas weight > 0, whose solution is free up to a constant per channel -- is solved on the
    mean-free vectors and the result keeps the mean of the start vector (f, or 0 without f); sequential channels only;
    any other operator is refused (capi.CcpError, UNSUPPORTED).  integrate_gradients is the front end for it.

    One operator per channel.  If any of wx, wy, data_weight is H x W x C, channel c is solved with channel c's weights
    (H x W arguments beside it serve every channel), and equals, bit for bit, the one-channel call on channel c's slices.
    A mini-batch of N single-channel images with their own weights is H x W x N with channels="batched": one PCG loop
    whose launches serve the whole batch, every image stopping at its own iteration."""
    import torch
    out_dtype = torch.uint8 if out_dtype is None else out_dtype
    ref = next((t for t in (f, gx, gy) if t is not None), None)
    if ref is None:
        raise ValueError("weighted_solve needs at least one of gx, gy, f")
    dev = _device_index(ref)
    H, W = ref.shape[0], ref.shape[1]
    C = ref.shape[2] if ref.dim() == 3 else 1
    g = capi.Grid(W, H, C, device=dev, weighted=True)
    g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
    try:
        g.mg_configure(hierarchy=hierarchy, precision=precision, channels=channels, smoother=smoother, nullspace=nullspace)
        _set_operator(g, _weight(wx, H, W, dev), _weight(wy, H, W, dev), _weight(data_weight, H, W, dev))
        g.assemble_weighted_rhs_tensor(gx, gy, f, init_x=f is not None)
        if f is None:
            g.fill_x(0.0)
        g.mg_conjugate_gradient(epsilon, iterations, 2)
        if out_dtype == torch.uint8:
            return g.store_u8_tensor()
        return g.get_x_tensor(dtype=out_dtype)
    finally:
        g.close()


def _no_nullspace(nullspace, who):
    if capi.mg_nullspace_value(nullspace) != capi.MG_NULLSPACES["none"]:
        raise ValueError(f"{who} does not take nullspace={nullspace!r}: a floating system has no fixed pixel, and the adjoint of "
                         "a floating solve is not implemented; use weighted_solve or integrate_gradients")


def integrate_gradients(gx, gy, wx=None, wy=None, mean=0.0, iterations: int = 200, epsilon: float = 1e-10, out_dtype=None,
                        hierarchy="galerkin", precision="f64", smoother="point"):
    """The image whose forward differences are closest to a gradient field: u minimises
    sum wx (u(x+1,y) - u(x,y) - gx)^2 + sum wy (u(x,y+1) - u(x,y) - gy)^2 per channel over the whole canvas with a free
    border (pure Neumann), which fixes u up to a constant; the constant is chosen so that mean(u) = `mean`.  gx, gy:
    float32 H x W x C (or H x W) device tensors, one may be None; wx, wy: H x W (or H x W x C: one operator per channel)
    float32 / float64 tensors or scalars, every in-canvas weight > 0 (None: 1); mean: a number, or one value per channel (a
    sequence or a tensor of C entries).  Solved on a weighted grid handle in its "constant" null-space mode
    (capi.Grid.mg_set_nullspace) by multigrid-preconditioned CG from u = mean: at most `iterations` iterations, to
    sqrt(r'r) < epsilon * |b| of the channel with the largest |b| (b = -div(w g), the mean of b removed); a field whose b is
    zero in every channel gives the constant image `mean` without a solve.  smoother="line" is refused on elongated
    canvases whose hierarchy has a line-smoothed level of one row or one column (capi.Grid.mg_set_nullspace).  Returns a device
    tensor of gx's shape, float64 unless out_dtype says otherwise (torch.uint8: clamped).  hierarchy, precision, smoother: as
    weighted_solve's; the channels are solved one after the other."""
    import torch
    ref = next((t for t in (gx, gy) if t is not None), None)
    if ref is None:
        raise ValueError("integrate_gradients needs at least one of gx, gy")
    if ref.dim() == 2:
        u = integrate_gradients(None if gx is None else gx.unsqueeze(-1), None if gy is None else gy.unsqueeze(-1), wx, wy, mean, iterations,
                                epsilon, out_dtype, hierarchy, precision, smoother)
        return u[..., 0]
    out_dtype = torch.float64 if out_dtype is None else out_dtype
    dev = _device_index(ref)
    H, W, C = ref.shape
    device = torch.device("cuda", dev)
    m = torch.as_tensor(mean, dtype=torch.float64, device=device).reshape(-1)
    if m.numel() not in (1, C):
        raise ValueError(f"mean must be a number or have one entry per channel ({C}), not {m.numel()}")
    g = capi.Grid(W, H, C, device=dev, weighted=True)
    g.set_stream(torch.cuda.current_stream(device).cuda_stream)
    try:
        g.mg_configure(hierarchy=hierarchy, precision=precision, smoother=smoother, nullspace="constant")
        _set_operator(g, _weight(wx, H, W, dev), _weight(wy, H, W, dev), None)
        g.assemble_weighted_rhs_tensor(gx, gy, None, init_x=False)
        g.set_x_tensor(m.reshape(1, 1, -1).expand(H, W, C).contiguous())
        _, bb = g.residual_norm2()
        if float(bb.max()) > 0.0:                          # b = 0 (a zero field, or every weighted gradient 0): u = mean as it stands
            g.mg_conjugate_gradient(epsilon * float(bb.max()) ** 0.5, iterations, 0)
        if out_dtype == torch.uint8:
            return g.store_u8_tensor()
        return g.get_x_tensor(dtype=out_dtype)
    finally:
        g.close()


def wls_weights(image, lam: float = 1.0, alpha: float = 1.2, eps: float = 1e-4):
    """The edge weights of WLS edge-preserving smoothing (Farbman et al. 2008) for a u8 or float H x W (x C) tensor:
    wx = lam / (|d/dx log(L + eps)|^alpha + eps), wy likewise, L the channel mean (u8 scaled to [0, 1]).  float64
    H x W tensors; the last column of wx and the last row of wy are never read (set to 0)."""
    import torch
    img = image.to(torch.float64)
    if image.dtype == torch.uint8:
        img = img / 255.0
    lum = img.mean(dim=-1) if img.dim() == 3 else img
    ell = torch.log(lum + eps)
    wx = torch.zeros_like(ell)
    wy = torch.zeros_like(ell)
    wx[:, :-1] = lam / (torch.abs(ell[:, 1:] - ell[:, :-1]) ** alpha + eps)
    wy[:-1, :] = lam / (torch.abs(ell[1:, :] - ell[:-1, :]) ** alpha + eps)
    return wx, wy


def wls_smooth(image, iterations: int, lam: float = 1.0, alpha: float = 1.2, eps: float = 1e-4, epsilon: float = 1e-10,
               hierarchy="galerkin", precision="f64", channels="sequential", smoother="point"):
    """WLS edge-preserving smoothing (Farbman et al. 2008): u minimises sum (u - image)^2 + sum wx (du/dx)^2 +
    sum wy (du/dy)^2 with wls_weights (torch ops: plumbing), solved on a weighted grid handle.  image: u8 or float
    H x W (x C) tensor; returns the same dtype and shape (u8: clamped).  hierarchy, precision, channels, smoother: as
    weighted_solve's."""
    import torch
    wx, wy = wls_weights(image, lam, alpha, eps)
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    out_dtype = torch.uint8 if image.dtype == torch.uint8 else image.dtype
    u = weighted_solve(None, None, f, iterations, wx=wx, wy=wy, data_weight=1.0, out_dtype=out_dtype, epsilon=epsilon,
                       hierarchy=hierarchy, precision=precision, channels=channels, smoother=smoother)
    return u if image.dim() == 3 else u[..., 0]


def constrained_solve(gx, gy, f, values, fixed, iterations: int, wx=None, wy=None, data_weight=None, out_dtype=None,
                      epsilon: float = 1e-10, hierarchy="rescaled", precision="f64", channels="sequential",
                      smoother="point", nullspace="none"):
    """weighted_solve with hard constraints: the pixels where `fixed` (an H x W uint8, bool, float32 or float64 tensor) is
    non-zero keep the value `values` prescribes (u8 / float32 / float64 H x W x C, None: 0) and the energy of
    weighted_solve is minimised over the others; edges that leave the canvas are absent, so the free region may touch
    the canvas border.  The mask stays on the device: it is read by the kernel that forms the operator and never copied
    to the host.  The start vector is f on the free pixels (0 without f).  Returns the composite -- the solution on the
    free pixels, `values` on the fixed ones -- as out_dtype (torch.uint8 by default: clamped).  With data_weight None or
    0 every connected set of free pixels needs a fixed neighbour, or the system is singular there.  precision, channels, smoother: as
    weighted_solve's.  wx, wy, data_weight or fixed given as H x W x C: one operator (and one fixed set) per channel, as
    in weighted_solve.  nullspace: "none" only (ValueError otherwise: a floating system has no fixed pixel)."""
    import torch
    _no_nullspace(nullspace, "constrained_solve")
    out_dtype = torch.uint8 if out_dtype is None else out_dtype
    dev = _device_index(fixed)
    H, W = fixed.shape[0], fixed.shape[1]
    ref = next((t for t in (values, f, gx, gy) if t is not None), None)
    C = ref.shape[2] if ref is not None and ref.dim() == 3 else 1
    g = capi.Grid(W, H, C, device=dev, weighted=True)
    g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
    try:
        g.mg_configure(hierarchy=hierarchy, precision=precision, channels=channels, smoother=smoother)
        _set_operator(g, _weight(wx, H, W, dev), _weight(wy, H, W, dev), _weight(data_weight, H, W, dev), fixed)
        if f is None:
            g.fill_x(0.0)
        g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=f is not None)
        g.mg_conjugate_gradient(epsilon, iterations, 2)
        if out_dtype == torch.uint8:
            return g.store_u8_tensor()
        return g.get_x_tensor(dtype=out_dtype)
    finally:
        g.close()


def clone_gradients(source, target=None):
    """The guidance field of seamless cloning as float32 H x W x C forward differences (torch ops: plumbing): the source's,
    or with `target` whichever of the two images' differences is larger in magnitude (ties take the source).  The last
    column of gx and the last row of gy are 0 (never read)."""
    import torch
    s = source.to(torch.float32)
    gx, gy = torch.zeros_like(s), torch.zeros_like(s)
    gx[:, :-1] = s[:, 1:] - s[:, :-1]
    gy[:-1] = s[1:] - s[:-1]
    if target is not None:
        t = target.to(torch.float32)
        tx, ty = t[:, 1:] - t[:, :-1], t[1:] - t[:-1]
        gx[:, :-1] = torch.where(tx.abs() > gx[:, :-1].abs(), tx, gx[:, :-1])
        gy[:-1] = torch.where(ty.abs() > gy[:-1].abs(), ty, gy[:-1])
    return gx, gy


def seamless_clone_constrained(source, target, mask, iterations: int, mixed: bool = False, data_weight=None, precision="f64",
                               channels="sequential", smoother="point", nullspace="none"):
    """Seamless cloning (Perez et al. 2003) on a weighted handle with fixed pixels: inside `mask` (H x W, non-zero = region)
    the result follows the gradients of the u8 H x W x C tensor `source` (mixed: the stronger of source's and target's),
    outside it is `target`.  Unlike seamless_clone the region may touch the canvas border (no condition is imposed there)
    and the mask stays on the device.  data_weight (a scalar or an H x W tensor) > 0 also pulls the region towards the
    source's colours (screened cloning).  The start vector is the target; multigrid-preconditioned CG, at most
    `iterations` iterations (precision: "f64" or "f32", the V-cycle's: capi.Grid.mg_set_precision; channels: "sequential" or
    "batched", capi.Grid.mg_set_channels; smoother: "point" or "line", capi.Grid.mg_set_smoother).  Returns the composite,
    a u8 H x W x C tensor.  nullspace: "none" only (ValueError otherwise)."""
    import torch
    _no_nullspace(nullspace, "seamless_clone_constrained")
    if source.dim() == 2:
        return seamless_clone_constrained(source.unsqueeze(-1), target.unsqueeze(-1), mask, iterations, mixed, data_weight, precision, channels, smoother)[..., 0]
    dev = _device_index(target)
    H, W, C = target.shape
    gx, gy = clone_gradients(source, target if mixed else None)
    fixed = mask == 0
    g = capi.Grid(W, H, C, device=dev, weighted=True)
    g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
    try:
        g.mg_configure(hierarchy="rescaled", precision=precision, channels=channels, smoother=smoother)
        g.set_weights_tensor(None, None, _weight(data_weight, H, W, dev), fixed=fixed)
        g.set_x_u8_tensor(target)
        g.assemble_constrained_rhs_tensor(gx, gy, None if data_weight is None else source, target, init_x=False)
        g.mg_conjugate_gradient(1e-10, iterations, 2)
        return g.store_u8_tensor()
    finally:
        g.close()


# ---- differentiable weighted solves -----------------------------------------------------------------------------------
_GRAD_INPUTS = ("gx", "gy", "f", "wx", "wy", "lam", "values")


def _converged(reports, what, strict):
    if strict and not all(r.converged for r in reports):
        its = [int(r.iterations) for r in reports]
        raise RuntimeError(f"weighted_solve_grad: the {what} solve did not converge (iterations per channel {its}); the "
                           "gradient of an unconverged solve is not the gradient: raise `iterations`, loosen `epsilon`, or pass strict=False")


def _solve_function():
    """The torch.autograd.Function behind weighted_solve_grad (built on first use: torch is imported lazily here)."""
    global _WeightedSolve
    if _WeightedSolve is not None:
        return _WeightedSolve
    import weakref

    import torch
    from torch.autograd.function import once_differentiable

    class WeightedSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, gx, gy, f, wx, wy, lam, values, fixed, cfg):
            ref = next(t for t in (values, f, gx, gy) if t is not None)
            dev = _device_index(ref)
            H, W = ref.shape[0], ref.shape[1]
            C = ref.shape[2] if ref.dim() == 3 else 1
            g = capi.Grid(W, H, C, device=dev, weighted=True)
            try:
                g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
                g.mg_configure(hierarchy=cfg["hierarchy"], precision=cfg["precision"], channels=cfg["channels"], smoother=cfg["smoother"])
                _set_operator(g, wx, wy, lam, fixed)
                if f is None:
                    g.fill_x(0.0)
                g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=f is not None)
                _converged(g.mg_conjugate_gradient(cfg["epsilon"], cfg["iterations"], 2), "forward", cfg["strict"])
                u = g.get_x_tensor()
            except BaseException:
                g.close()
                raise
            # The handle lives as long as autograd keeps this node's saved tensors: `token` is saved with them, and
            # its finaliser closes the handle when they are released -- after a backward without retain_graph, or when
            # the graph is dropped without a backward.
            token = torch.empty(0, device=u.device)
            weakref.finalize(token, g.close)
            ctx.grid, ctx.cfg = g, cfg
            ctx.present = [t is not None for t in (gx, gy, f, wx, wy, lam, values, fixed)]
            ctx.save_for_backward(*[t for t in (gx, gy, f, wx, wy, lam, values, fixed) if t is not None], u, token)
            return u if ref.dim() == 3 else u[..., 0]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            saved = list(ctx.saved_tensors)
            u = saved[-2]
            it = iter(saved[:-2])
            gx, gy, f, wx, wy, lam, values, fixed = [next(it) if p else None for p in ctx.present]
            g, cfg = ctx.grid, ctx.cfg
            want = tuple(n for n, need in zip(_GRAD_INPUTS, ctx.needs_input_grad[:7]) if need)
            grad = grad.reshape(u.shape)
            if grad.dtype not in (torch.float32, torch.float64):
                grad = grad.to(torch.float64)
            g.set_stream(torch.cuda.current_stream(u.device).cuda_stream)
            g.adjoint_begin_tensor(grad)
            _converged(g.mg_conjugate_gradient(cfg["epsilon"], cfg["iterations"], 2), "adjoint", cfg["strict"])
            inputs = dict(gx=gx, gy=gy, f=f, wx=wx, wy=wy, lam=lam, values=values)
            out = {}
            for n in want:                                 # each gradient in its input's dtype and shape
                t = inputs[n]
                out[n] = torch.empty(t.shape, dtype=t.dtype, device=t.device)
            got = g.weighted_adjoint_tensor(u, grad if "values" in want else None, gx, gy, f, wx, wy, lam, fixed, want=want, out=out)
            return tuple(got.get(n) for n in _GRAD_INPUTS) + (None, None)

    _WeightedSolve = WeightedSolve
    return WeightedSolve


_WeightedSolve = None


def weighted_solve_grad(gx, gy, f, iterations: int, wx=None, wy=None, data_weight=None, values=None, fixed=None,
                        epsilon: float = 1e-10, hierarchy="rescaled", precision="f64", channels="sequential", smoother="point",
                        strict: bool = True, nullspace="none"):
    """weighted_solve / constrained_solve as a differentiable torch function: returns x, a float64 H x W x C tensor (the
    composite: the minimiser on the free pixels, `values` on the fixed ones) with a grad_fn, so that a loss of x can be
    differentiated with respect to gx, gy, f, wx, wy, data_weight and values.  Inputs as constrained_solve's (`fixed` None:
    no fixed pixels); wx, wy, data_weight may also be python scalars (no gradient) or 0-dim tensors, which are expanded to
    H x W here, outside the autograd function, so that torch sums their gradient to a scalar.  u8 inputs get no gradient.

    Backward.  The operator is symmetric, so the backward pass is one more multigrid PCG on the same handle -- same
    hierarchy, precision, channel mode and smoother, the same epsilon and iteration cap -- with dL/dx as the right-hand
    side (v: A v = dL/dx on the free pixels, 0 on fixed ones), then one kernel pass for all channels that forms only the
    gradients autograd asks for (s_x = v(x+1,y) - v(x,y), r_x = gx - (x(x+1,y) - x(x,y)), likewise to the south):
        d/dwx = sum_c s_x r_x    d/dgx = wx s_x    d/ddata_weight = sum_c v (f - x)   (0 at fixed pixels)
        d/dwy = sum_c s_y r_y    d/dgy = wy s_y    d/df = data_weight v               (0 at fixed pixels)
        d/dvalues = dL/dx + the four-neighbour sum of w v at fixed pixels, 0 at free pixels
    each returned in its input's dtype.  The operator is never formed again.  Backward is once-differentiable.

    Memory.  The grid handle -- x, b, the operator planes, the multigrid hierarchy and the PCG vectors, about what the
    forward solve itself held -- and x stay in device memory until backward has run (with retain_graph=True: until the
    graph is dropped); it is released as soon as autograd releases the node's saved tensors.  Under torch.no_grad(), or
    when no input requires a gradient, use weighted_solve / constrained_solve, which release it at once.

    One operator per channel.  If any of wx, wy, data_weight, fixed is H x W x C the handle gets one operator per channel
    (weighted_solve): an H x W x C weight gets an H x W x C gradient, channel c's from channel c alone (no sum over
    channels), equal to the gradient of the one-channel call on channel c's slices; an H x W weight or a scalar passed
    beside it is expanded to H x W x C here, outside the autograd function, so that torch sums its gradient over the
    channels through the broadcast.  A mini-batch of N single-channel images with their own weights is H x W x N with
    channels="batched".

    strict (the default): a forward or adjoint solve that does not report `converged` within `iterations` raises
    RuntimeError -- these are the gradients of the converged solution, and an unconverged solve's are not them.

    nullspace: "none" only (ValueError otherwise): the adjoint of a floating solve is out of scope."""
    import torch
    _no_nullspace(nullspace, "weighted_solve_grad")
    ref = next((t for t in (values, f, gx, gy) if t is not None), None)
    if ref is None:
        raise ValueError("weighted_solve_grad needs at least one of gx, gy, f, values")
    dev = _device_index(ref)
    H, W = ref.shape[0], ref.shape[1]

    C = ref.shape[2] if ref.dim() == 3 else 1
    stacked = _per_channel(wx, wy, data_weight, fixed)

    def plane(w):
        if isinstance(w, torch.Tensor) and w.dim() == 0:
            w = w.expand(H, W)
        w = _weight(w, H, W, dev)
        if stacked and w is not None and w.dim() == 2:
            w = w.unsqueeze(-1).expand(H, W, C)
        return w

    cfg = dict(iterations=int(iterations), epsilon=float(epsilon), hierarchy=hierarchy, precision=precision, channels=channels,
               smoother=smoother, strict=bool(strict))
    return _solve_function().apply(gx, gy, f, plane(wx), plane(wy), plane(data_weight), values, fixed, cfg)


# ---- a persistent weighted handle: prepare once, then only enqueue ------------------------------------------------------
class WeightedSolver:
    """A weighted grid handle that lives across solves, for loops that solve many right-hand sides on ONE operator (a
    training loop, a video, the replays of a torch.cuda.graph).  The functions above create a handle per call, and their
    solve waits for the host; here set_operator pays for everything that allocates or synchronises -- the operator's
    validation, the multigrid hierarchy, the PCG vectors (capi.Grid.mg_prepare) -- and solve / solve_grad then only
    enqueue on torch's current stream (capi.Grid.mg_conjugate_gradient_enqueue): no host synchronisation and no
    allocation on the handle, so a solve may be recorded by torch.cuda.graph together with whatever produces its inputs
    and consumes its result.  refresh_operator gives the installed operator new values the same way, enqueue only, so
    weights that a network or a reweighting step produces every step can sit in the same graph; refresh_constraints does the
    same with a new mask of fixed pixels, on a handle whose constraint planes exist (reserve_constraints before set_operator).
    reweight IS such a reweighting step: it forms the weights on the device from the last solution (irls_solve, tv_denoise).

    H, W, C: the canvas and its channels; device: a torch device or a GPU index.  iterations: every solve enqueues
    exactly this many PCG iterations (<= 4096); a channel that reaches sqrt(r'r) < epsilon earlier stops there and the
    remaining launches are no-ops for it, so x and the report are those of the synchronous solve with the same cap, bit
    for bit (`iterations` in a report counts completed iterations, and the update that passes epsilon is one more: a system
    that reports 6 needs iterations >= 7 here).  epsilon is absolute until set_stop gives a relative tolerance: then every
    solve, forward or adjoint, stops channel c at sqrt(r'r) < max(epsilon, relative * |b_c|), |b_c| of the right-hand side
    that solve finds on the device (capi.Grid.mg_conjugate_gradient_enqueue_relative).
    hierarchy, precision, channels, smoother, nullspace: as weighted_solve's (the hierarchy defaults to "rescaled", as in weighted_solve_grad).  Two smoothing sweeps, as everywhere in this module.

    Nothing checks convergence for you -- that would be a read-back: pass `report` (a float64 C x 6 tensor: iterations,
    converged, last_l1_step, b_mean, x_mean, 0 per channel; C x 8 with a relative tolerance set: then |b_c| and the
    threshold follow) and look at it when the stream has passed."""

    SWEEPS = 2

    def __init__(self, H, W, C, device, *, iterations, epsilon, hierarchy="rescaled", precision="f64", channels="sequential",
                 smoother="point", nullspace="none"):
        import torch
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type != "cuda":
            raise ValueError("WeightedSolver needs a GPU device")
        dev = device.index if device.index is not None else torch.cuda.current_device()
        if not 0 <= int(iterations) <= 4096:
            raise ValueError(f"iterations must be 0 .. 4096 (one call queues exactly that many), not {iterations}")
        self.H, self.W, self.C, self.device = int(H), int(W), int(C), torch.device("cuda", dev)
        self.iterations, self.epsilon = int(iterations), float(epsilon)
        self.relative = None                               # set_stop: the tolerance relative to |b|, or None (epsilon alone)
        self.nullspace = capi.mg_nullspace_value(nullspace)
        self._operator = None
        self._planes = False                               # refresh_constraints has run: the constraint planes exist
        self._generation = 0                               # refreshes of the handle's operator so far (solve_grad's backward)
        self._zero = torch.zeros((), dtype=torch.float64, device=self.device).expand(self.H, self.W, self.C)
        self.grid = capi.Grid(self.W, self.H, self.C, device=dev, weighted=True)
        try:
            self.grid.mg_configure(hierarchy=hierarchy, precision=precision, channels=channels, smoother=smoother, nullspace=nullspace)
        except BaseException:
            self.grid.close()
            raise

    def set_operator(self, wx, wy, data_weight=None, fixed=None):
        """Install the operator (wx, wy, data_weight: H x W tensors or scalars, None: 1, 1, 0; fixed: an H x W mask of
        prescribed pixels or None; any of them H x W x C: one operator per channel, chosen as weighted_solve chooses)
        and prepare the solve for it.  Synchronises; raises capi.CcpError for a refused operator or mode combination.
        Not to be called while a stream is being captured."""
        dev = self.device.index
        wx, wy, lam = (_weight(w, self.H, self.W, dev) for w in (wx, wy, data_weight))
        self._operator = None
        self._planes = False
        _set_operator(self.grid, wx, wy, lam, fixed)
        self.grid.mg_prepare(self.SWEEPS)
        self._operator = (wx, wy, lam, fixed)

    def set_stop(self, epsilon=None, relative=None):
        """The stop test of every later solve, solve_grad's forward and backward included.  epsilon: the absolute tolerance
        (None: keep the present one).  relative: None -- the state after __init__ -- stops at sqrt(r'r) < epsilon and
        reports C x 6, as ever; a number stops channel c at sqrt(r'r) < max(epsilon, relative * |b_c|), with |b_c| the norm
        of the right-hand side of THAT solve, formed on the device: of the assembled system in a forward solve, of dL/du
        in a backward one, whatever the scale of the loss.  Reports and adjoint reports are then C x 8 (|b_c| and the
        threshold follow the six fields).  Give epsilon a floor where a right-hand side may vanish.  Host state only:
        nothing is enqueued, and a solve already recorded in a graph keeps the test it was recorded with."""
        if epsilon is not None:
            self.epsilon = float(epsilon)
        self.relative = None if relative is None else float(relative)

    def _enqueue_pcg(self, report):
        """The enqueue solve on what the handle holds, by the stop test set_stop chose."""
        if self.relative is None:
            return self.grid.mg_conjugate_gradient_enqueue(self.epsilon, self.iterations, self.SWEEPS, report)
        return self.grid.mg_conjugate_gradient_enqueue_relative(self.epsilon, self.relative, self.iterations, self.SWEEPS, report)

    def _enqueue_solve(self, gx, gy, f, values, x0, out, report):
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        g = self.grid
        g.set_x_tensor(self._zero if x0 is None else x0)
        g.assemble_constrained_rhs_tensor(gx, gy, f, values, init_x=False)   # (puts `values` on the fixed pixels of x)
        self._enqueue_pcg(report)
        return g.get_x_tensor(out=out)

    def solve(self, gx, gy, f, values=None, x0=None, out=None, report=None):
        """Minimise weighted_solve's / constrained_solve's energy for the installed operator: the right-hand side from gx,
        gy (float32 H x W x C or None), f and values (u8 / float32 / float64 or None), x from x0 (float32 / float64
        H x W x C) or 0, the solve, and x copied into `out` (float32 / float64 H x W x C; a new float64 tensor when None).
        Returns (out, report).  Enqueue only."""
        return self._enqueue_solve(gx, gy, f, values, x0, out, report), report

    def refresh_operator(self, wx, wy, data_weight=None):
        """New values for the installed operator (wx, wy, data_weight as set_operator's; None: 1, 1, 0), enqueued on torch's
        current stream (capi.Grid.refresh_weights_tensor): no synchronisation and no allocation on the handle, so it may
        be recorded by torch.cuda.graph in front of a solve.  The fixed pixels, the kind of the operator (an H x W x C weight
        needs an operator installed per channel; H x W weights serve either kind) and every mode stay: set_operator remains
        the synchronising call and the only one that changes those.  (A python scalar becomes a new device tensor here: inside
        a capture pass tensors.)  Bad weights are not raised here -- that would be a
        read-back: the solves then leave x alone and field 5 of their report carries the status
        (capi.Grid.operator_status reads it, synchronising)."""
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        dev = self.device.index
        wx, wy, lam = (_weight(w, self.H, self.W, dev) for w in (wx, wy, data_weight))
        self.grid.refresh_weights_tensor(wx, wy, lam)
        self._operator = (wx, wy, lam, self._operator[3])
        self._generation += 1

    def reweight(self, penalty, coupling, scale, epsilon, u=None, gx=None, gy=None, base_wx=None, base_wy=None, data_weight=None, out=None,
                 *, data_penalty=None, data_scale=1.0, data_epsilon=None, f=None):
        """refresh_operator with weights formed on the device from the current solution, the reweighting step of an IRLS
        loop (capi.Grid.reweight_tensor): w = base * (scale * phi(q)) per edge, q the squared residual of the edge against
        gx / gy summed over the channels (all of them on a shared operator, channel c alone on an operator per channel).
        penalty: "charbonnier" | "huber" | "reciprocal"; coupling: "edge" | "pixel"; u: None reads the handle's x -- the
        last solve's solution -- else a u8 / float32 / float64 H x W x C tensor (a guide, or f for the first step);
        base_wx, base_wy, data_weight: as refresh_operator's wx, wy, data_weight (None: 1, 1, 0).  Enqueue only, as
        refresh_operator: it may be recorded by torch.cuda.graph between two solves.  Returns (wx, wy), the weights formed:
        `out` if given (a pair of float32 / float64 tensors, H x W on a shared operator, H x W x C on one per channel), else
        two new float64 tensors (inside a capture pass `out`).  They are recorded as the installed weights, so a later
        solve_grad's backward re-installs the right ones.  They carry no grad_fn: reweight_grad is this call as a
        differentiable function, and irls_solve_grad the whole outer loop.

        data_penalty (keyword only): None makes exactly the call above.  "charbonnier" | "huber" | "reciprocal" |
        "quadratic" reweights the data term in the same pass (capi.Grid.reweight_robust_tensor): per pixel
        lambda = data_weight * (data_scale * phi_d(dq)), dq the sum of (f - u)^2 over the channels of the operator, phi_d on
        data_epsilon (data_weight None: 1 there; "quadratic": phi_d = 1, f and data_epsilon are not read; `penalty` may
        then be "quadratic" as well).  Returns (wx, wy, lam), `out` then a pair as above or a triple; the lambda formed is
        recorded as the installed one, for solve_grad's backward."""
        import torch
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        if data_penalty is None:
            capi.reweight_ids(penalty, coupling)
        else:
            capi.robust_ids(penalty, coupling, data_penalty)
        dev = self.device.index
        bwx, bwy, lam = (_weight(w, self.H, self.W, dev) for w in (base_wx, base_wy, data_weight))
        n_out = 2 if data_penalty is None else 3
        if out is None or len(out) < n_out:
            shape = (self.H, self.W, self.C) if self.grid.operator_channels() > 1 else (self.H, self.W)
            with torch.cuda.device(self.device):
                out = tuple(out or ()) + tuple(torch.empty(shape, dtype=torch.float64, device=self.device) for _ in range(n_out - len(out or ())))
        if data_penalty is not None:
            wx, wy, formed = out
            self.grid.reweight_robust_tensor(penalty, coupling, scale, epsilon, data_penalty, data_scale, data_epsilon, f=f, u=u, gx=gx, gy=gy,
                                             base_wx=bwx, base_wy=bwy, lam=lam, out_wx=wx, out_wy=wy, out_lambda=formed)
            self._operator = (wx, wy, formed, self._operator[3])
            self._generation += 1
            return wx, wy, formed
        wx, wy = out
        self.grid.reweight_tensor(penalty, coupling, scale, epsilon, u=u, gx=gx, gy=gy, base_wx=bwx, base_wy=bwy, lam=lam, out_wx=wx, out_wy=wy)
        self._operator = (wx, wy, lam, self._operator[3])
        self._generation += 1
        return wx, wy

    def reweight_grad(self, penalty, coupling, scale, epsilon, u, gx=None, gy=None, base_wx=None, base_wy=None, data_weight=None, *,
                      data_penalty=None, data_scale=1.0, data_epsilon=None, f=None):
        """reweight as a differentiable function: it installs the weights exactly as reweight does (the same call, the same
        bits) and returns them -- (wx, wy), or (wx, wy, lam) with data_penalty -- as new float64 tensors with a grad_fn, so
        that solve_grad(wx=, wy=, data_weight=) on them unrolls an IRLS step that autograd can differentiate.  u: a tensor,
        required (the image the weights are formed from: f for the first step, the previous step's result later).
        Backward is one launch (capi.Grid.reweight_adjoint_tensor) and once-differentiable; it returns gradients for u, gx,
        gy, base_wx, base_wy and, with data_penalty, data_weight and f, each in its input's dtype and shape.  u8 inputs and
        python scalars get none; scale, the epsilons and data_scale get none (a learnable strength is a base weight with
        scale 1).  A 0-dim tensor is expanded to H x W and, on an operator per channel, an H x W tensor to H x W x C here,
        outside the autograd function, so that torch sums its gradient: solve_grad's rule.  Without data_penalty lambda is
        not formed here: data_weight passes through to the handle, and its gradient is solve_grad(data_weight=)'s alone.
        The tensors saved for backward are the inputs; nothing of the handle's state is needed then, so several forwards
        may precede their backwards."""
        import torch
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        if data_penalty is None:
            capi.reweight_ids(penalty, coupling)
        else:
            capi.robust_ids(penalty, coupling, data_penalty)
        if not isinstance(u, torch.Tensor):
            raise ValueError("reweight_grad needs u, the tensor the weights are formed from")
        stacked = self.grid.operator_channels() > 1 or _per_channel(base_wx, base_wy, data_weight)

        def plane(w):
            if isinstance(w, torch.Tensor) and w.dim() == 0:
                w = w.expand(self.H, self.W)
            w = _weight(w, self.H, self.W, self.device.index)
            if stacked and w is not None and w.dim() == 2:
                w = w.unsqueeze(-1).expand(self.H, self.W, self.C)
            return w

        def image(t):
            if isinstance(t, torch.Tensor) and t.dim() == 2:
                t = t.unsqueeze(-1).expand(self.H, self.W, self.C)
            return t

        cfg = dict(penalty=penalty, coupling=coupling, scale=float(scale), epsilon=float(epsilon), data_penalty=data_penalty,
                   data_scale=float(data_scale), data_epsilon=data_epsilon)
        return _reweight_function().apply(image(u), gx, gy, plane(base_wx), plane(base_wy), plane(data_weight), image(f), self, cfg)

    def reserve_constraints(self):
        """Before set_operator: keep the handle's constraint planes whether or not the operator fixes a pixel
        (capi.Grid.reserve_constraints), so that refresh_constraints may give it a fixed set later.  Results are unchanged
        bit for bit; 24 bytes per pixel and operator.  Host state only."""
        self.grid.reserve_constraints(True)

    def refresh_constraints(self, wx, wy, data_weight=None, fixed=None):
        """refresh_operator with a new set of fixed pixels (fixed: as set_operator's, None: no pixel fixed), enqueued on
        torch's current stream (capi.Grid.refresh_constrained_tensor): no synchronisation and no allocation on the handle,
        so a mask per frame, sample or brush stroke can sit in the same torch.cuda.graph as the solve.  Needs the
        constraint planes: reserve_constraints() before set_operator, or a set_operator whose mask fixed a pixel.  The kind
        of the operator and every mode stay.  Nothing is raised for bad weights, as in refresh_operator."""
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        dev = self.device.index
        wx, wy, lam = (_weight(w, self.H, self.W, dev) for w in (wx, wy, data_weight))
        self.grid.refresh_constrained_tensor(wx, wy, lam, fixed)
        self._operator = (wx, wy, lam, fixed)
        self._planes = True
        self._generation += 1

    def solve_grad(self, gx, gy, f, values=None, x0=None, report=None, adjoint_report=None, *, wx=None, wy=None, data_weight=None):
        """solve as a differentiable function of gx, gy, f and values (weighted_solve_grad's formulas).  Returns (u, report),
        u a new float64 H x W x C tensor with a grad_fn.  Backward is the adjoint right-hand side, one more enqueue solve and
        the gradient pass on this same handle; it needs only the saved u and inputs, so several forwards may precede their
        backwards.  No `strict` check: the adjoint solve's figures land in `adjoint_report` if given.

        wx, wy, data_weight (keyword only): when any is given, forward first refreshes the operator with them
        (refresh_operator; the ones not given keep the installed operator's values) and backward also returns their
        gradients, by weighted_solve_grad's formulas and rules: each in its input's dtype and shape, python scalars get
        none, a 0-dim tensor is expanded to H x W outside the autograd function so that torch sums its gradient, and on an
        operator per channel an H x W weight is expanded to H x W x C the same way.  If the handle's operator has been
        refreshed again since this forward, backward first refreshes it with the weights it saved, so forwards on
        different weights may precede their backwards.  Without the three the function is what it was, bit for bit (no
        gradients for the installed weights: weighted_solve_grad or these keywords are for those)."""
        if self.nullspace != capi.MG_NULLSPACES["none"]:
            _no_nullspace("constant", "WeightedSolver.solve_grad")
        weights = (None, None, None)
        if wx is not None or wy is not None or data_weight is not None:
            import torch
            if self._operator is None:
                raise RuntimeError("WeightedSolver: set_operator first")
            stacked = self.grid.operator_channels() > 1 or _per_channel(wx, wy, data_weight)

            def plane(w, installed):
                if w is None:                              # (no gradient for a weight the caller did not hand in)
                    return installed.detach() if isinstance(installed, torch.Tensor) else installed
                if isinstance(w, torch.Tensor) and w.dim() == 0:
                    w = w.expand(self.H, self.W)
                w = _weight(w, self.H, self.W, self.device.index)
                if stacked and w.dim() == 2:
                    w = w.unsqueeze(-1).expand(self.H, self.W, self.C)
                return w

            weights = tuple(plane(w, old) for w, old in zip((wx, wy, data_weight), self._operator[:3]))
        return _persistent_function().apply(gx, gy, f, values, x0, *weights, self, report, adjoint_report, weights != (None, None, None)), report

    def fixed_point_grad(self, u, penalty, coupling, scale, epsilon, gx, gy, f, values=None, base_wx=None, base_wy=None, data_weight=None, *,
                         backward_steps, backward_tolerance=None, check_every=8, backward_history=None, strict=True, data_penalty=None,
                         data_scale=1.0, data_epsilon=None):
        """Attach the gradient of an IRLS fixed point to u: u is taken to be a fixed point of the step u -> solve(w(u)) on this
        solver (the loop of irls_solve run until it stopped moving; the reweight's arguments, gx, gy, f, values and the
        base weights as that loop took them), and the call returns u unchanged -- the same storage, detached -- with a
        grad_fn towards gx, gy, f, values, base_wx, base_wy and data_weight.  The forward installs w(u)
        (reweight(u=u): one launch) and saves u and the inputs, nothing else: no iterate, no weights, so the memory does not
        depend on how many steps produced u.  u8 inputs and python numbers get no gradient; a 0-dim tensor is expanded to
        H x W and, on an operator per channel, an H x W tensor to H x W x C outside the autograd function (reweight_grad's rule).

        Backward (once-differentiable, enqueue only unless backward_tolerance is given).  With G = dL/du and J the Jacobian
        of one IRLS step at u, z = (I - J')^-1 G is reached by z_0 = G, z_{k+1} = G + J'z_k:
          1. if a later call has moved the handle's operator, w(u) is installed again (reweight(u=u));
          2. adjoint_begin with G and one enqueue solve: v = A^-1 z_0;
          3. `backward_steps` times: the fused step (capi.Grid.irls_adjoint_step_tensor: z := G + J'z from v, in one launch),
             then an enqueue solve to the solver's stop test, warm-started from the previous v;
          4. the gradient pass and the reweight's adjoint once, for the parameter gradients, each in its input's dtype
             and shape (float32 ones are formed in float64 and rounded once).
        The z iteration converges at the forward loop's own linear rate -- on 16 x 12 x 2, epsilon 5e-2: 35 forward steps
        to an update of 1e-12 and 36 backward steps to the same relative change; Huber / edge 49 and 50, TV-L1 19 and 16 --
        so backward_steps of about the forward's step count is the natural choice.  A finite backward_steps is a truncated
        Neumann series: the gradient lacks the terms beyond J'^backward_steps.  "reciprocal" carries no convexity guarantee,
        and with it neither loop need converge.
        backward_tolerance: None -- no synchronisation; a number: the step's report is read every `check_every` steps
        and the loop ends once ||z_new - z_old|| <= backward_tolerance * ||G||; with `strict`, RuntimeError if
        backward_steps is reached first.  backward_history: None, or a list that receives one channels x 2 report tensor
        per step made, (sum (z_new - z_old)^2, sum z_new^2) per channel.
        data_penalty, data_scale, data_epsilon: the robust data term, as reweight's (data_weight is then the base lambda).
        The gradient is that of the fixed point: where u is not one -- the forward loop stopped early -- it is wrong by
        O(||u_K - u_{K-1}||)."""
        import torch
        if self.nullspace != capi.MG_NULLSPACES["none"]:
            _no_nullspace("constant", "WeightedSolver.fixed_point_grad")
        if self._operator is None:
            raise RuntimeError("WeightedSolver: set_operator first")
        if data_penalty is None:
            capi.reweight_ids(penalty, coupling)
        else:
            capi.robust_ids(penalty, coupling, data_penalty)
        if not isinstance(u, torch.Tensor) or f is None:
            raise ValueError("fixed_point_grad needs u, the fixed point, and f")
        if int(backward_steps) < 0 or int(check_every) < 1:
            raise ValueError("backward_steps must be >= 0 and check_every >= 1")
        stacked = self.grid.operator_channels() > 1 or _per_channel(base_wx, base_wy, data_weight)

        def plane(w):
            if isinstance(w, torch.Tensor) and w.dim() == 0:
                w = w.expand(self.H, self.W)
            w = _weight(w, self.H, self.W, self.device.index)
            if stacked and w is not None and w.dim() == 2:
                w = w.unsqueeze(-1).expand(self.H, self.W, self.C)
            return w

        def image(t):
            if isinstance(t, torch.Tensor) and t.dim() == 2:
                t = t.unsqueeze(-1).expand(self.H, self.W, self.C)
            return t

        cfg = dict(penalty=penalty, coupling=coupling, scale=float(scale), epsilon=float(epsilon), data_penalty=data_penalty,
                   data_scale=float(data_scale), data_epsilon=data_epsilon, steps=int(backward_steps),
                   tolerance=None if backward_tolerance is None else float(backward_tolerance), check_every=int(check_every),
                   history=backward_history, strict=bool(strict))
        return _fixed_point_function().apply(image(u.detach()), gx, gy, image(f), image(values), plane(base_wx), plane(base_wy),
                                             plane(data_weight), self, cfg)

    def close(self):
        self.grid.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _irls_steps(s, gx, gy, f, values, x, outer, penalty, coupling, strength, epsilon, base_wx, base_wy, lam, robust, data_penalty, first_step,
                history, last_report=None):
    """irls_solve's loop on solver `s` from x: `outer` x (reweight -- step 0 from f, step k from the handle's x -- then the
    warm-started solve).  last_report: None, or a C x 8 tensor for the last step's report where `history` is None.  Returns
    (x, the x the last step started from).  Enqueue only."""
    import torch
    before = x
    for k in range(int(outer)):
        if data_penalty is not None:
            robust["data_penalty"] = "quadratic" if k == 0 and first_step == "quadratic" else data_penalty
        w = s.reweight(penalty, coupling, strength, epsilon, u=f if k == 0 else None, gx=gx, gy=gy, base_wx=base_wx, base_wy=base_wy,
                       data_weight=lam, **robust)
        report = None if history is None else torch.zeros((s.C, 8), dtype=torch.float64, device=x.device)
        if report is None and k == int(outer) - 1:
            report = last_report
        before = x
        x, _ = s.solve(gx, gy, f, values, x0=x, report=report)
        if history is not None:
            history.append((x, report) + tuple(w))
    return x, before


def irls_solve(gx, gy, f, outer: int, iterations: int, penalty="charbonnier", coupling="edge", strength=1.0, epsilon=1e-2, data_weight=1.0,
               wx=None, wy=None, fixed=None, values=None, tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential",
               smoother="point", out_dtype=None, history=None, data_penalty=None, data_epsilon=None, first_step="quadratic"):
    """Robust gradient-domain fitting by iteratively reweighted least squares: `outer` steps of (reweight, assemble, solve)
    on one WeightedSolver, every step a launch sequence -- after set_operator nothing synchronises until the caller reads
    the result.  It minimises
        E(u) = sum over edges 2 strength base psi(rho) + sum data_weight (u - f)^2,   psi'(rho) = rho phi(rho^2),
    rho = sqrt(q) the residual of the edge (WeightedSolver.reweight: gx - (uE - u) over the channels, gy to the south):
        "charbonnier": phi = 1 / sqrt(rho^2 + epsilon^2),   psi = sqrt(rho^2 + epsilon^2)
        "huber":       phi = 1 / max(rho, epsilon),          psi = rho^2 / (2 epsilon) for rho < epsilon, rho - epsilon / 2 beyond
        "reciprocal":  phi = 1 / (rho + epsilon),            psi = rho - epsilon log(1 + rho / epsilon)
    coupling "edge" takes every edge's own rho (anisotropic: with zero guidance sum |du/dx| + |du/dy|); "pixel" takes
    rho^2 = q_x + q_y per pixel for both of its forward edges and the sum then runs over pixels (isotropic; the energy
    reading needs wx = wy there).  Each psi(sqrt(t)) is concave in t, so the weighted least-squares problem of a step
    majorises E at the current iterate and E does not increase from step to step (up to the inner tolerance).
    gx, gy: float32 H x W x C or None (0); f: u8 / float32 / float64 H x W x C, the data term and the first step's u (the
    later steps reweight from the handle's x); wx, wy (the base weights), data_weight, fixed, values: as
    WeightedSolver.set_operator's and solve's (an H x W x C weight: one operator per channel, each channel its own rho).
    Every step solves warm-started from the previous solution, at most `iterations` PCG iterations to
    sqrt(r'r) < tolerance * |b|.  history: None, or a list that receives one (u, report, wx, wy) of device tensors per
    outer step (report C x 8, WeightedSolver.set_stop's; wx, wy the weights the step solved with): convergence is not
    checked here, that would be a read-back.  Returns x as out_dtype (None: torch.uint8, clamped, for a u8 f, else float64).
    The result carries no grad_fn: irls_solve_grad is this loop unrolled for autograd (WeightedSolver.reweight_grad and
    solve_grad(wx=, wy=)), with the same values.  Strongly varying weights -- small epsilon, sharp edges -- are where smoother="line" helps.

    data_penalty: None -- the quadratic data term above, and exactly the calls made before this argument existed -- or
    "charbonnier" | "huber" | "reciprocal": the data term is robust as well, and every step reweights the edges and lambda
    in one call (WeightedSolver.reweight(data_penalty=...)).  The loop then minimises
        E(u) = sum over edges 2 strength base psi(rho) + sum over pixels 2 data_weight psi_d(delta),
    delta^2 = sum over the channel set of (u - f)^2 (all channels on a shared operator, channel c alone on an operator per
    channel), psi_d the penalty above on data_epsilon; psi_d(sqrt(t)) is concave as well, so the step's least-squares
    problem still majorises E.  data_weight: a python number is the call's data_scale (lambda = data_weight * phi_d), a
    tensor its base lambda with data_scale 1.  first_step: the first step reweights from u = f, where every data residual is
    0 and a robust lambda would be data_weight * phi_d(0) everywhere -- data_weight / data_epsilon, a uniform weight that
    depends on data_epsilon and knows nothing of the outliers; "quadratic" (the default) therefore gives step 0 the quadratic data term
    (data_penalty "quadratic": lambda = data_weight) and "robust" the robust one.  The step-0 problem of "quadratic"
    majorises another energy, so the descent property holds from the second step on.  history entries are then
    (u, report, wx, wy, lam), lam the lambda the step solved with."""
    import torch
    if data_penalty is None:
        capi.reweight_ids(penalty, coupling)
    else:
        capi.robust_ids(penalty, coupling, data_penalty)
        if data_penalty == "quadratic" or penalty == "quadratic":
            raise ValueError('irls_solve: "quadratic" is data_penalty=None (and no edge penalty); WeightedSolver.reweight takes it')
        if first_step not in ("quadratic", "robust"):
            raise ValueError(f'first_step must be "quadratic" or "robust", not {first_step!r}')
        if data_epsilon is None:
            raise ValueError("irls_solve: a robust data term needs data_epsilon")
    if f is None:
        raise ValueError("irls_solve needs f: the data term, and the image the first step reweights from")
    if int(outer) < 1:
        raise ValueError(f"outer must be at least 1, not {outer}")
    dev = _device_index(f)
    H, W = f.shape[0], f.shape[1]
    C = f.shape[2] if f.dim() == 3 else 1
    if out_dtype is None:
        out_dtype = torch.uint8 if f.dtype == torch.uint8 else torch.float64
    with WeightedSolver(H, W, C, dev, iterations=iterations, epsilon=0.0, hierarchy=hierarchy, precision=precision, channels=channels,
                        smoother=smoother) as s:
        s.set_operator(wx, wy, data_weight, fixed)
        s.set_stop(relative=tolerance)
        base_wx, base_wy, lam, _ = s._operator
        x = f.to(torch.float64).reshape(H, W, C)
        robust = {}
        if data_penalty is not None:
            scalar = not isinstance(data_weight, torch.Tensor)
            robust = dict(data_scale=float(data_weight) if scalar else 1.0, data_epsilon=data_epsilon, f=f)
            if scalar:
                lam = None
        x, _ = _irls_steps(s, gx, gy, f, values, x, outer, penalty, coupling, strength, epsilon, base_wx, base_wy, lam, robust, data_penalty,
                           first_step, history)
        if out_dtype == torch.uint8:
            return s.grid.store_u8_tensor()
        return x if out_dtype == torch.float64 else x.to(out_dtype)


def tv_denoise(image, strength, outer: int = 10, iterations: int = 400, epsilon=1e-2, isotropic=True, data_weight=1.0, tolerance=1e-10,
               hierarchy="rescaled", precision="f64", channels="sequential", smoother="point", history=None):
    """Total-variation denoising (Rudin, Osher, Fatemi 1992) by irls_solve: u minimises
    2 strength TV_epsilon(u) + sum data_weight (u - image)^2 with the Charbonnier-smoothed total variation -- isotropic:
    sum over pixels sqrt(|grad u|^2 + epsilon^2), the gradient over all channels (vectorial TV); isotropic=False: the
    anisotropic sum over edges sqrt(du^2 + epsilon^2).  Zero guidance, f = image, "pixel" or "edge" coupling.  image: a u8 or
    float H x W (x C) tensor; strength and epsilon are in the image's own units (a u8 image: grey levels).  Returns the
    image's dtype and shape (u8: clamped, as wls_smooth).  The other arguments are irls_solve's."""
    import torch
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    out_dtype = torch.uint8 if image.dtype == torch.uint8 else image.dtype
    u = irls_solve(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge", strength=strength,
                   epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy, precision=precision, channels=channels,
                   smoother=smoother, out_dtype=out_dtype, history=history)
    return u if image.dim() == 3 else u[..., 0]


def tv_l1_denoise(image, strength, outer: int = 12, iterations: int = 400, epsilon=1e-2, data_epsilon=5e-2, isotropic=True, data_weight=1.0,
                  tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential", smoother="point", first_step="quadratic",
                  history=None):
    """TV-L1 denoising by irls_solve: tv_denoise with the data term an L1 norm as well, u minimises
    2 strength TV_epsilon(u) + 2 data_weight sum over pixels sqrt(|u - image|^2 + data_epsilon^2), both Charbonnier-smoothed,
    |u - image| over all channels.  Where tv_denoise follows an outlier -- salt and pepper, a dead pixel -- as hard as its
    square, this replaces it from its neighbourhood.  image, strength, epsilon, isotropic and the return value: as
    tv_denoise's; data_epsilon: in the image's own units, as epsilon; first_step and the other arguments: irls_solve's
    (history entries carry the lambda of each step)."""
    import torch
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    out_dtype = torch.uint8 if image.dtype == torch.uint8 else image.dtype
    u = irls_solve(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge", strength=strength,
                   epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy, precision=precision, channels=channels,
                   smoother=smoother, out_dtype=out_dtype, history=history, data_penalty="charbonnier", data_epsilon=data_epsilon,
                   first_step=first_step)
    return u if image.dim() == 3 else u[..., 0]


def irls_solve_grad(gx, gy, f, outer: int, iterations: int, penalty="charbonnier", coupling="edge", strength=1.0, epsilon=1e-2, data_weight=1.0,
                    wx=None, wy=None, fixed=None, values=None, tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential",
                    smoother="point", history=None, data_penalty=None, data_epsilon=None, first_step="quadratic", strict: bool = True,
                    adjoint_history=None):
    """irls_solve unrolled for autograd: the same `outer` x (reweight, assemble, solve) on one WeightedSolver, through
    reweight_grad and solve_grad(wx=, wy=, data_weight=).  Returns x, a float64 H x W x C tensor with a grad_fn towards gx, gy,
    f, values, wx, wy (the base weights), a tensor data_weight and a tensor strength; u8 inputs and python numbers get no
    gradient.  Step 0 reweights from f, step k from step k - 1's returned tensor, which holds the handle's x: with a
    python-number strength the calls are irls_solve's and a refresh with the weights just formed, and x has irls_solve's bits.
    Arguments as irls_solve's (no out_dtype: float64); a 0-dim wx, wy or data_weight is expanded to H x W.

    strength: a python number is the reweight's scale, as in irls_solve.  A 0-dim tensor is folded into the base weights --
    base = strength.expand(H, W), times wx / wy where given -- with scale 1.0, so that its gradient is the sum of the base
    weights' gradients and needs no read-back (the weights then differ from the number's in the last bits).

    Backward walks the steps in reverse: per step the adjoint right-hand side, one more enqueue solve to the same relative
    tolerance, the gradient pass, and one launch for the adjoint of the reweight.  It is enqueue-only; adjoint_history: None,
    or a list that receives `outer` C x 8 report tensors here, each filled when its step's backward has run.
    strict (the default): the `outer` forward reports are read back once after the loop -- the one synchronisation -- and a
    solve that did not converge raises RuntimeError: the gradient of an unconverged solve is not the gradient.
    history: as irls_solve's.

    Memory.  Per outer step u, wx, wy (and lam) stay alive until backward, beside the inputs, and the handle -- x, b, the
    operator planes, the hierarchy and the PCG vectors -- lives as long as the graph does.  irls_solve_implicit
    differentiates the loop at its fixed point instead: the converged solution's gradient, from u and the inputs alone."""
    import torch
    if data_penalty is None:
        capi.reweight_ids(penalty, coupling)
    else:
        capi.robust_ids(penalty, coupling, data_penalty)
        if data_penalty == "quadratic" or penalty == "quadratic":
            raise ValueError('irls_solve_grad: "quadratic" is data_penalty=None (and no edge penalty); WeightedSolver.reweight_grad takes it')
        if first_step not in ("quadratic", "robust"):
            raise ValueError(f'first_step must be "quadratic" or "robust", not {first_step!r}')
        if data_epsilon is None:
            raise ValueError("irls_solve_grad: a robust data term needs data_epsilon")
    if f is None:
        raise ValueError("irls_solve_grad needs f: the data term, and the image the first step reweights from")
    if int(outer) < 1:
        raise ValueError(f"outer must be at least 1, not {outer}")
    dev = _device_index(f)
    H, W = f.shape[0], f.shape[1]
    if f.dim() == 2:
        f = f.unsqueeze(-1)
    C = f.shape[2]
    flat = lambda w: w.expand(H, W) if isinstance(w, torch.Tensor) and w.dim() == 0 else w
    wx, wy, data_weight = flat(wx), flat(wy), flat(data_weight)
    s = WeightedSolver(H, W, C, dev, iterations=iterations, epsilon=0.0, hierarchy=hierarchy, precision=precision, channels=channels,
                       smoother=smoother)              # (not closed here: backward needs it; it goes with the graph)
    try:
        s.set_operator(wx, wy, data_weight, fixed)
        s.set_stop(relative=tolerance)
        base_wx, base_wy, lam, _ = s._operator
        scale = strength
        if isinstance(strength, torch.Tensor):
            if strength.dim() != 0:
                raise ValueError("a tensor strength must be 0-dim")
            scale = 1.0
            base_wx = strength.expand(H, W) if wx is None else strength * wx
            base_wy = strength.expand(H, W) if wy is None else strength * wy
        robust = {}
        if data_penalty is not None:
            scalar = not isinstance(data_weight, torch.Tensor)
            robust = dict(data_scale=float(data_weight) if scalar else 1.0, data_epsilon=data_epsilon, f=f)
            if scalar:
                lam = None
        x = f.detach().to(torch.float64)
        u_in, reports = f, []
        for k in range(int(outer)):
            if data_penalty is not None:
                robust["data_penalty"] = "quadratic" if k == 0 and first_step == "quadratic" else data_penalty
            w = s.reweight_grad(penalty, coupling, scale, epsilon, u_in, gx=gx, gy=gy, base_wx=base_wx, base_wy=base_wy, data_weight=lam, **robust)
            report, adjoint = (torch.zeros((C, 8), dtype=torch.float64, device=x.device) for _ in range(2))
            # the data weight of the solve: the lambda just formed, else the caller's tensor (a number stays the installed one)
            solve_lam = w[2] if data_penalty is not None else (lam if isinstance(data_weight, torch.Tensor) else None)
            u_in, _ = s.solve_grad(gx, gy, f, values, x0=x, report=report, adjoint_report=adjoint, wx=w[0], wy=w[1], data_weight=solve_lam)
            x = u_in.detach()
            reports.append(report)
            if adjoint_history is not None:
                adjoint_history.append(adjoint)
            if history is not None:
                history.append((x, report) + tuple(t.detach() for t in w))
        if strict and not bool(torch.stack(reports)[:, :, 1].all()):
            its = [[int(i) for i in r[:, 0].tolist()] for r in reports]
            raise RuntimeError(f"irls_solve_grad: a forward solve did not converge (iterations per step and channel {its}); the gradient "
                               "of an unconverged solve is not the gradient: raise `iterations`, loosen `tolerance`, or pass strict=False")
        return u_in
    except BaseException:
        s.close()
        raise


def tv_denoise_grad(image, strength, outer: int = 10, iterations: int = 400, epsilon=1e-2, isotropic=True, data_weight=1.0, tolerance=1e-10,
                    hierarchy="rescaled", precision="f64", channels="sequential", smoother="point", history=None, strict: bool = True,
                    adjoint_history=None):
    """tv_denoise as a differentiable function of the image, of a 0-dim tensor strength and of a tensor data_weight
    (irls_solve_grad: zero guidance, f = image, Charbonnier, "pixel" or "edge" coupling).  Returns float64, the image's shape."""
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    u = irls_solve_grad(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge", strength=strength,
                        epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy, precision=precision,
                        channels=channels, smoother=smoother, history=history, strict=strict, adjoint_history=adjoint_history)
    return u if image.dim() == 3 else u[..., 0]


def tv_l1_denoise_grad(image, strength, outer: int = 12, iterations: int = 400, epsilon=1e-2, data_epsilon=5e-2, isotropic=True, data_weight=1.0,
                       tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential", smoother="point", first_step="quadratic",
                       history=None, strict: bool = True, adjoint_history=None):
    """tv_l1_denoise as a differentiable function, as tv_denoise_grad is tv_denoise's (the data term Charbonnier on
    data_epsilon as well).  Returns float64, the image's shape."""
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    u = irls_solve_grad(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge", strength=strength,
                        epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy, precision=precision,
                        channels=channels, smoother=smoother, history=history, data_penalty="charbonnier", data_epsilon=data_epsilon,
                        first_step=first_step, strict=strict, adjoint_history=adjoint_history)
    return u if image.dim() == 3 else u[..., 0]


_ReweightGrad = None


def _reweight_function():
    """The torch.autograd.Function behind WeightedSolver.reweight_grad (built on first use, as _solve_function)."""
    global _ReweightGrad
    if _ReweightGrad is not None:
        return _ReweightGrad
    import torch
    from torch.autograd.function import once_differentiable

    names = ("u", "gx", "gy", "base_wx", "base_wy", "lam", "f")

    class ReweightGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, u, gx, gy, base_wx, base_wy, lam, f, solver, cfg):
            robust = {}
            if cfg["data_penalty"] is not None:
                robust = dict(data_penalty=cfg["data_penalty"], data_scale=cfg["data_scale"], data_epsilon=cfg["data_epsilon"], f=f)
            w = solver.reweight(cfg["penalty"], cfg["coupling"], cfg["scale"], cfg["epsilon"], u=u, gx=gx, gy=gy, base_wx=base_wx,
                                base_wy=base_wy, data_weight=lam, **robust)
            ctx.solver, ctx.cfg = solver, cfg
            ctx.present = [t is not None for t in (u, gx, gy, base_wx, base_wy, lam, f)]
            ctx.save_for_backward(*[t for t in (u, gx, gy, base_wx, base_wy, lam, f) if t is not None])
            return tuple(w)

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            it = iter(ctx.saved_tensors)
            inputs = {n: next(it) if p else None for n, p in zip(names, ctx.present)}
            cfg = ctx.cfg
            with_data = cfg["data_penalty"] is not None
            want = tuple(n for n, need in zip(names, ctx.needs_input_grad[:7])
                         if need and inputs[n] is not None and (with_data or n not in ("lam", "f")))
            got = {}
            if want:
                floats = (torch.float32, torch.float64)
                grads = [None if g is None else (g if g.dtype in floats else g.to(torch.float64)) for g in grads]
                out = {n: torch.empty(inputs[n].shape, dtype=inputs[n].dtype, device=inputs[n].device) for n in want}
                robust = {}
                if with_data:
                    robust = dict(data_penalty=cfg["data_penalty"], data_scale=cfg["data_scale"], data_epsilon=cfg["data_epsilon"],
                                  f=inputs["f"], grad_lambda=grads[2])
                got = ctx.solver.grid.reweight_adjoint_tensor(cfg["penalty"], cfg["coupling"], cfg["scale"], cfg["epsilon"], inputs["u"],
                                                              gx=inputs["gx"], gy=inputs["gy"], base_wx=inputs["base_wx"],
                                                              base_wy=inputs["base_wy"], lam=inputs["lam"], grad_wx=grads[0],
                                                              grad_wy=grads[1], want=want, out=out, **robust)
            return tuple(got.get(n) for n in names) + (None, None)

    _ReweightGrad = ReweightGrad
    return ReweightGrad


_PersistentSolve = None


def _persistent_function():
    """The torch.autograd.Function behind WeightedSolver.solve_grad (built on first use, as _solve_function)."""
    global _PersistentSolve
    if _PersistentSolve is not None:
        return _PersistentSolve
    import torch
    from torch.autograd.function import once_differentiable

    names = ("gx", "gy", "f", "values", "wx", "wy", "lam")

    class PersistentSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, gx, gy, f, values, x0, wx, wy, lam, solver, report, adjoint_report, refresh):
            if refresh:                                    # (a weight the caller did not give arrives as the installed one)
                solver.refresh_operator(wx, wy, lam)
            u = solver._enqueue_solve(gx, gy, f, values, x0, None, report)
            ctx.solver, ctx.adjoint_report = solver, adjoint_report
            ctx.generation = solver._generation
            # the operator this solve ran on: what backward hands the gradient pass, and refreshes the handle with if
            # another refresh has happened in between
            wx, wy, lam, ctx.fixed = solver._operator
            ctx.present = [t is not None for t in (gx, gy, f, values, wx, wy, lam)]
            ctx.save_for_backward(*[t for t in (gx, gy, f, values, wx, wy, lam) if t is not None], u)
            return u

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            saved = list(ctx.saved_tensors)
            u = saved[-1]
            it = iter(saved[:-1])
            inputs = {n: next(it) if p else None for n, p in zip(names, ctx.present)}
            solver = ctx.solver
            g = solver.grid
            wx, wy, lam, fixed = inputs["wx"], inputs["wy"], inputs["lam"], ctx.fixed
            if solver._generation != ctx.generation:       # the handle holds a later refresh's values: back to this solve's
                if solver._planes:                         # ... and perhaps a later mask: weights and mask
                    solver.refresh_constraints(wx, wy, lam, fixed)
                else:
                    solver.refresh_operator(wx, wy, lam)
                ctx.generation = solver._generation
            need = list(ctx.needs_input_grad[:4]) + list(ctx.needs_input_grad[5:8])
            want = tuple(n for n, yes in zip(names, need) if yes)
            grad = grad.reshape(u.shape)
            if grad.dtype not in (torch.float32, torch.float64):
                grad = grad.to(torch.float64)
            g.adjoint_begin_tensor(grad)
            solver._enqueue_pcg(ctx.adjoint_report)
            out = {n: torch.empty(inputs[n].shape, dtype=inputs[n].dtype, device=inputs[n].device) for n in want}
            got = g.weighted_adjoint_tensor(u, grad if "values" in want else None, inputs["gx"], inputs["gy"], inputs["f"], wx, wy, lam,
                                            fixed, want=want, out=out)
            return tuple(got.get(n) for n in names[:4]) + (None,) + tuple(got.get(n) for n in names[4:]) + (None, None, None, None)

    _PersistentSolve = PersistentSolve
    return PersistentSolve


_FixedPointGrad = None


def _fixed_point_function():
    """The torch.autograd.Function behind WeightedSolver.fixed_point_grad (built on first use, as _solve_function)."""
    global _FixedPointGrad
    if _FixedPointGrad is not None:
        return _FixedPointGrad
    import torch
    from torch.autograd.function import once_differentiable

    names = ("gx", "gy", "f", "values", "base_wx", "base_wy", "lam")

    def install(solver, cfg, u, t):
        """reweight(u=u): the operator A(w(u)) on the handle; and, where a later call may have moved the mask too, the mask"""
        robust = {}
        if cfg["data_penalty"] is not None:
            robust = dict(data_penalty=cfg["data_penalty"], data_scale=cfg["data_scale"], data_epsilon=cfg["data_epsilon"], f=t["f"])
        fixed = solver._operator[3]
        w = solver.reweight(cfg["penalty"], cfg["coupling"], cfg["scale"], cfg["epsilon"], u=u, gx=t["gx"], gy=t["gy"], base_wx=t["base_wx"],
                            base_wy=t["base_wy"], data_weight=t["lam"], **robust)
        return fixed, w

    class FixedPointGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, u, gx, gy, f, values, base_wx, base_wy, lam, solver, cfg):
            t = dict(zip(names, (gx, gy, f, values, base_wx, base_wy, lam)))
            ctx.fixed, _ = install(solver, cfg, u, t)
            ctx.solver, ctx.cfg, ctx.generation = solver, cfg, solver._generation
            ctx.present = [v is not None for v in t.values()]
            ctx.save_for_backward(*[v for v in t.values() if v is not None], u)
            return u.detach()

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            saved = list(ctx.saved_tensors)
            u = saved[-1]
            it = iter(saved[:-1])
            t = {n: next(it) if p else None for n, p in zip(names, ctx.present)}
            solver, cfg = ctx.solver, ctx.cfg
            g = solver.grid
            robust = cfg["data_penalty"] is not None
            if solver._generation != ctx.generation:       # the handle holds a later call's operator: back to w(u)
                _, w = install(solver, cfg, u, t)
                if solver._planes:                         # ... and perhaps a later mask
                    solver.refresh_constraints(w[0], w[1], w[2] if robust else t["lam"], ctx.fixed)
                ctx.generation = solver._generation
            wx, wy, lam_op, fixed = solver._operator
            grad = grad.reshape(u.shape)
            if grad.dtype not in (torch.float32, torch.float64):
                grad = grad.to(torch.float64)
            how = dict(gx=t["gx"], gy=t["gy"], base_wx=t["base_wx"], base_wy=t["base_wy"], lam=t["lam"])
            if robust:
                how.update(data_penalty=cfg["data_penalty"], data_scale=cfg["data_scale"], data_epsilon=cfg["data_epsilon"], f=t["f"])
            args = (cfg["penalty"], cfg["coupling"], cfg["scale"], cfg["epsilon"], u)
            g.adjoint_begin_tensor(grad)
            solver._enqueue_pcg(None)
            tol, history = cfg["tolerance"], cfg["history"]
            shared = torch.zeros((solver.C, 2), dtype=torch.float64, device=u.device) if tol is not None and history is None else None
            bound = None if tol is None else tol * tol * float(grad.to(torch.float64).pow(2).sum())
            done = tol is None
            for k in range(cfg["steps"]):
                report = shared
                if history is not None:
                    report = torch.zeros((solver.C, 2), dtype=torch.float64, device=u.device)
                    history.append(report)
                g.irls_adjoint_step_tensor(*args, grad, fixed=fixed, report=report, **how)
                solver._enqueue_pcg(None)
                if tol is not None and ((k + 1) % cfg["check_every"] == 0 or k + 1 == cfg["steps"]):
                    if float(report[:, 0].sum()) <= bound:   # (the one read-back per check)
                        done = True
                        break
            if not done and cfg["strict"]:
                raise RuntimeError(f"fixed_point_grad: the adjoint iteration did not reach backward_tolerance {tol} within {cfg['steps']} "
                                   "steps; raise backward_steps, loosen backward_tolerance, or pass strict=False")
            need = dict(zip(names, ctx.needs_input_grad[1:8]))
            need = {n: bool(y) and t[n] is not None for n, y in need.items()}
            # the gradient pass: the weights' gradients always (the reweight's adjoint is fed with them), the rest as asked
            want = ("wx", "wy", "lam") + tuple(n for n in ("gx", "gy", "f") if need[n])
            got = g.weighted_adjoint_tensor(u, None, t["gx"], t["gy"], t["f"], wx, wy, lam_op, fixed, want=want)
            back_names = {"gx": "gx", "gy": "gy", "base_wx": "base_wx", "base_wy": "base_wy"}
            if robust:
                back_names.update(f="f", lam="lam")
            want_back = ("u",) + tuple(m for n, m in back_names.items() if need[n])
            back = g.reweight_adjoint_tensor(*args, grad_wx=got["wx"], grad_wy=got["wy"], grad_lambda=got["lam"] if robust else None,
                                             want=want_back, **how)
            out = {}
            for n in ("gx", "gy", "f"):
                if need[n]:
                    out[n] = got[n] + back[n] if n in back else got[n]
            for n in ("base_wx", "base_wy"):
                if need[n]:
                    out[n] = back[n]
            if need["lam"]:
                out["lam"] = back["lam"] if robust else got["lam"]
            if need["values"]:                             # z at every pixel, the fixed ones included: G + g_u of the last v
                z = grad.to(torch.float64) + back["u"]
                out["values"] = g.weighted_adjoint_tensor(u, z, t["gx"], t["gy"], t["f"], wx, wy, lam_op, fixed, want=("values",))["values"]
            grads = tuple(None if n not in out else out[n].to(t[n].dtype).reshape(t[n].shape) for n in names)
            return (None,) + grads + (None, None)

    _FixedPointGrad = FixedPointGrad
    return FixedPointGrad


def irls_solve_implicit(gx, gy, f, outer: int, iterations: int, penalty="charbonnier", coupling="edge", strength=1.0, epsilon=1e-2,
                        data_weight=1.0, wx=None, wy=None, fixed=None, values=None, tolerance=1e-10, hierarchy="rescaled", precision="f64",
                        channels="sequential", smoother="point", history=None, data_penalty=None, data_epsilon=None, first_step="quadratic",
                        strict: bool = True, backward_steps=None, backward_tolerance=None, check_every: int = 8, backward_history=None):
    """irls_solve differentiated at its fixed point instead of unrolled: the forward is irls_solve's own loop on one
    WeightedSolver under torch.no_grad() -- warm-started, enqueue only, no autograd node per step, the value irls_solve's bit
    for bit (with a python-number strength) -- and WeightedSolver.fixed_point_grad then gives the result a grad_fn towards
    gx, gy, f, values, wx, wy (the base weights), a tensor data_weight and a 0-dim tensor strength.  Returns float64 H x W x C.
    Arguments as irls_solve_grad's; strength as there (a 0-dim tensor is folded into the base weights with scale 1).

    The gradient is that of the FIXED POINT, the minimiser the loop converges to, not of the `outer`-step truncation
    irls_solve_grad differentiates; where the forward has not converged it is wrong by O(||u_K - u_{K-1}||).  strict (the
    default): the last forward step's update is read once -- the one synchronisation of the forward -- and RuntimeError is
    raised unless ||u_K - u_{K-1}|| <= tolerance * ||u_K|| and the last solve reports converged.  Memory: u and the inputs
    are saved, whatever `outer` is; the handle lives as long as the graph does.

    backward_steps (None: `outer`), backward_tolerance, check_every, backward_history: fixed_point_grad's.  The z iteration
    of the backward converges at the forward's own linear rate (on 16 x 12 x 2, epsilon 5e-2, TV: 35 forward steps to an
    update of 1e-12, 36 backward steps to the same relative change; Huber / edge 49 and 50; TV-L1 19 and 16), and a finite
    backward_steps is a truncated Neumann series.  "reciprocal" carries no convexity guarantee: neither loop need converge.
    What WeightedSolver.solve_grad refuses is refused here the same way."""
    import torch
    if data_penalty is None:
        capi.reweight_ids(penalty, coupling)
    else:
        capi.robust_ids(penalty, coupling, data_penalty)
        if data_penalty == "quadratic" or penalty == "quadratic":
            raise ValueError('irls_solve_implicit: "quadratic" is data_penalty=None (and no edge penalty)')
        if first_step not in ("quadratic", "robust"):
            raise ValueError(f'first_step must be "quadratic" or "robust", not {first_step!r}')
        if data_epsilon is None:
            raise ValueError("irls_solve_implicit: a robust data term needs data_epsilon")
    if f is None:
        raise ValueError("irls_solve_implicit needs f: the data term, and the image the first step reweights from")
    if int(outer) < 1:
        raise ValueError(f"outer must be at least 1, not {outer}")
    dev = _device_index(f)
    H, W = f.shape[0], f.shape[1]
    if f.dim() == 2:
        f = f.unsqueeze(-1)
    C = f.shape[2]
    flat = lambda w: w.expand(H, W) if isinstance(w, torch.Tensor) and w.dim() == 0 else w
    wx, wy, data_weight = flat(wx), flat(wy), flat(data_weight)
    scale, base_wx, base_wy = strength, wx, wy
    if isinstance(strength, torch.Tensor):
        if strength.dim() != 0:
            raise ValueError("a tensor strength must be 0-dim")
        scale = 1.0
        base_wx = strength.expand(H, W) if wx is None else strength * wx
        base_wy = strength.expand(H, W) if wy is None else strength * wy
    off = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    s = WeightedSolver(H, W, C, dev, iterations=iterations, epsilon=0.0, hierarchy=hierarchy, precision=precision, channels=channels,
                       smoother=smoother)              # (not closed here: backward needs it; it goes with the graph)
    try:
        scalar = not isinstance(data_weight, torch.Tensor)
        with torch.no_grad():
            s.set_operator(off(wx), off(wy), off(data_weight), fixed)
            s.set_stop(relative=tolerance)
            _, _, lam, _ = s._operator
            robust = {}
            if data_penalty is not None:
                robust = dict(data_scale=float(data_weight) if scalar else 1.0, data_epsilon=data_epsilon, f=off(f))
                if scalar:
                    lam = None
            report = torch.zeros((C, 8), dtype=torch.float64, device=f.device) if strict and history is None else None
            x, before = _irls_steps(s, off(gx), off(gy), off(f), off(values), off(f).to(torch.float64), outer, penalty, coupling, scale, epsilon,
                                    off(base_wx), off(base_wy), lam, robust, data_penalty, first_step, history, report)
            if strict:
                last = report if history is None else history[-1][1]
                moved, size, ok = torch.stack([(x - before).norm(), x.norm(), last[:, 1].min()]).tolist()
                if not ok or not moved <= tolerance * size:
                    raise RuntimeError(f"irls_solve_implicit: after {outer} steps the forward loop still moves by {moved:.3g} (||u|| = "
                                       f"{size:.3g}; last solve converged: {bool(ok)}): the fixed point's gradient is wrong by about that. "
                                       "Raise `outer` (or `iterations`), or pass strict=False")
            del report, before
        # the differentiable data weight: the caller's tensor (a number stays a number: no gradient, and the robust call's scale)
        grad_lam = data_weight if not scalar else (None if data_penalty is not None else lam)
        return s.fixed_point_grad(x, penalty, coupling, scale, epsilon, gx, gy, f, values, base_wx, base_wy, grad_lam,
                                  backward_steps=int(outer) if backward_steps is None else backward_steps, backward_tolerance=backward_tolerance,
                                  check_every=check_every, backward_history=backward_history, strict=strict,
                                  **({} if data_penalty is None else dict(data_penalty=data_penalty, data_scale=robust["data_scale"],
                                                                          data_epsilon=data_epsilon)))
    except BaseException:
        s.close()
        raise


def tv_denoise_implicit(image, strength, outer: int = 40, iterations: int = 400, epsilon=1e-2, isotropic=True, data_weight=1.0,
                        tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential", smoother="point", history=None,
                        strict: bool = True, backward_steps=None, backward_tolerance=None, check_every: int = 8, backward_history=None):
    """tv_denoise differentiated at its fixed point (irls_solve_implicit: zero guidance, f = image, Charbonnier, "pixel" or
    "edge" coupling): a differentiable function of the image, of a 0-dim tensor strength and of a tensor data_weight whose
    memory does not grow with `outer`.  The gradient is the fixed point's: wrong by O(||u_K - u_{K-1}||) where the forward
    has not converged, which strict (the default) checks with one read-back; a finite backward_steps (None: `outer`) is a
    truncated Neumann series that converges at the forward's rate.  Returns float64, the image's shape."""
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    u = irls_solve_implicit(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge",
                            strength=strength, epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy,
                            precision=precision, channels=channels, smoother=smoother, history=history, strict=strict,
                            backward_steps=backward_steps, backward_tolerance=backward_tolerance, check_every=check_every,
                            backward_history=backward_history)
    return u if image.dim() == 3 else u[..., 0]


def tv_l1_denoise_implicit(image, strength, outer: int = 40, iterations: int = 400, epsilon=1e-2, data_epsilon=5e-2, isotropic=True,
                           data_weight=1.0, tolerance=1e-10, hierarchy="rescaled", precision="f64", channels="sequential", smoother="point",
                           first_step="quadratic", history=None, strict: bool = True, backward_steps=None, backward_tolerance=None,
                           check_every: int = 8, backward_history=None):
    """tv_l1_denoise differentiated at its fixed point, as tv_denoise_implicit is tv_denoise's (the data term Charbonnier on
    data_epsilon as well); the same caveats: the fixed point's gradient, wrong by O(||u_K - u_{K-1}||) where the forward has
    not converged (strict checks it), and a truncated Neumann series for a finite backward_steps.  Returns float64, the
    image's shape."""
    f = image if image.dim() == 3 else image.unsqueeze(-1)
    u = irls_solve_implicit(None, None, f, outer, iterations, penalty="charbonnier", coupling="pixel" if isotropic else "edge",
                            strength=strength, epsilon=epsilon, data_weight=data_weight, tolerance=tolerance, hierarchy=hierarchy,
                            precision=precision, channels=channels, smoother=smoother, history=history, data_penalty="charbonnier",
                            data_epsilon=data_epsilon, first_step=first_step, strict=strict, backward_steps=backward_steps,
                            backward_tolerance=backward_tolerance, check_every=check_every, backward_history=backward_history)
    return u if image.dim() == 3 else u[..., 0]
