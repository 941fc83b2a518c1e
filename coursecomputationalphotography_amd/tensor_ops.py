"""Poisson solves on torch tensors: the tensor counterparts of the C++ facade's ccp::SolveChannel, ccp::BlendRegion
and ccp::SeamlessClone (include/ccp/photomontage.h), on the device hand-off of a grid handle (Grid.*_tensor).

Images stay on the GPU from input to result: the right-hand side is assembled from the tensors on the device, the
solve runs there, and the result is a u8 tensor on the same device.  Every call is enqueued on torch's current stream
of that device; the solvers themselves wait for their own reports, so the call returns once the solve is done.
`solver` takes the names of the facade's ccp::Solver: "GaussSeidel" (red-black), "ConjugateGradient",
"GaussSeidelReferenceOrder" and "MultigridConjugateGradient"; `iterations` means what it means there (fixed sweep
count for the Gauss-Seidel solvers, the iteration cap at epsilon 1e-10 for the CG solvers).
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
    g = capi.Grid(W, H, C, device=dev, mask=None if mask is None else _host_mask(mask))
    g.set_stream(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)
    return g


def _host_mask(mask) -> np.ndarray:
    import torch
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    return np.asarray(mask)


def solve_channels(gx, gy, constraint, iterations: int, init=None, solver: str = "GaussSeidel"):
    """Every channel of SolveChannel's system at once: b from float32 H x W x C gradient tensors and the pin values
    `constraint` (one int per channel), the start vector from the u8 H x W x C tensor `init` (the composite of
    fast_init_value) or, without it, 1.0 for Gauss-Seidel and 0 for CG, as the reference solvers start.  Returns the
    clamped solution as a u8 H x W x C tensor."""
    _check_solver(solver)
    dev = _device_index(gx)
    H, W = gx.shape[0], gx.shape[1]
    C = gx.shape[2] if gx.dim() == 3 else 1
    g = _grid(W, H, C, dev)
    try:
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
    a u8 H x W x C tensor.  The mask may be a tensor, but it is copied to the host once: the handle builds its
    region layout on the host."""
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
    H x W, copied to the host once (see blend_region); a region touching the canvas border raises CcpError.  Returns
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
