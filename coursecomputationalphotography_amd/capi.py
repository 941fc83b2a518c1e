"""ctypes binding of libccp_gs.so (the C ABI declared in include/ccp_gs.h).

This is plumbing for tests, bench.py and the multi-GPU driver: the product is the shared
library.  There is no CPU fallback — if the library is missing, or no HIP device is usable,
the calls raise (``CcpError``) instead of computing anything on the host.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import sys
import weakref
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CCP_GS_LIB: developer override to A/B two builds of the library in one session
LIB_PATH = os.environ.get("CCP_GS_LIB") or os.path.join(_HERE, "lib", "libccp_gs.so")

CCP_OK = 0
GRID_DIRICHLET_MASK = 1
GRID_WEIGHTED = 2
MG_HIERARCHY_GALERKIN, MG_HIERARCHY_RESCALED = 0, 1
MG_HIERARCHIES = {"galerkin": MG_HIERARCHY_GALERKIN, "rescaled": MG_HIERARCHY_RESCALED}
MG_PRECISIONS = {"f64": 0, "f32": 1}
MG_CHANNELS = {"sequential": 0, "batched": 1}
MG_SMOOTHERS = {"point": 0, "line": 1}
MG_NULLSPACES = {"none": 0, "constant": 1}
# The multigrid options of a grid handle, in the order Grid.mg_configure applies them: option -> (its names and their
# CCP_MG_* integers, whether an integer that is none of them is left to the library -- CcpError, not ValueError).  The
# C functions are ccp_grid_mg_set_<option> and ccp_grid_mg_get_<option>.
MG_OPTIONS = {"hierarchy": (MG_HIERARCHIES, True), "precision": (MG_PRECISIONS, True), "channels": (MG_CHANNELS, False),
              "smoother": (MG_SMOOTHERS, False), "nullspace": (MG_NULLSPACES, False)}


def _mg_value(option, value):
    """The CCP_MG_* integer of a name of `option` (or of one of its integers): ValueError otherwise."""
    names, any_integer = MG_OPTIONS[option]
    if isinstance(value, str):
        if value not in names:
            raise ValueError(f"{option} must be one of {sorted(names)}, not {value!r}")
        return names[value]
    if not any_integer and int(value) not in names.values():
        raise ValueError(f"{option} must be one of {sorted(names.values())}, not {value!r}")
    return int(value)


def mg_channels_value(mode):
    """The CCP_MG_CHANNELS_* integer of "sequential" / "batched" (or of an integer of MG_CHANNELS): ValueError otherwise."""
    return _mg_value("channels", mode)


def mg_smoother_value(kind):
    """The CCP_MG_SMOOTHER_* integer of "point" / "line" (or of an integer of MG_SMOOTHERS): ValueError otherwise."""
    return _mg_value("smoother", kind)


def mg_nullspace_value(kind):
    """The CCP_MG_NULLSPACE_* integer of "none" / "constant" (or of an integer of MG_NULLSPACES): ValueError otherwise."""
    return _mg_value("nullspace", kind)


ORDER_LEXICOGRAPHIC = 0
ORDER_MULTICOLOUR = 1
CLONE_IMPORT = 0
CLONE_MIXED = 1

# every symbol include/ccp_gs.h declares (tests check the library exports all of them)
ABI_SYMBOLS = (
    "ccp_status_string", "ccp_abi_version", "ccp_device_count",
    "ccp_csr_create", "ccp_csr_destroy", "ccp_csr_upload", "ccp_csr_upload_rows", "ccp_csr_rows_info", "ccp_csr_set_colouring", "ccp_csr_get_colouring", "ccp_csr_insert", "ccp_csr_insert_many", "ccp_csr_edit_stats", "ccp_csr_device_footprint", "ccp_csr_last_path", "ccp_csr_embed_region_host",
    "ccp_csr_gauss_seidel", "ccp_csr_conjugate_gradient", "ccp_csr_conjugate_gradient_jacobi", "ccp_csr_apply_to_vector", "ccp_csr_residual_norm2",
    "ccp_grid_create", "ccp_grid_destroy", "ccp_grid_get_layout", "ccp_grid_set_stream",
    "ccp_grid_synchronize", "ccp_grid_set_b_host", "ccp_grid_set_x_host", "ccp_grid_get_x_host",
    "ccp_grid_get_b_host", "ccp_grid_set_mask_host", "ccp_grid_fill_x", "ccp_grid_b_from_x", "ccp_grid_randomize_x",
    "ccp_grid_sweep", "ccp_grid_sweep_edges_first", "ccp_grid_stream_wait_edges", "ccp_grid_tune", "ccp_grid_set_fused", "ccp_grid_set_tiling", "ccp_grid_get_tiling", "ccp_grid_sweep_l1", "ccp_grid_halo_refreshed", "ccp_grid_gauss_seidel", "ccp_grid_gauss_seidel_lexicographic", "ccp_debug_lex_tickets", "ccp_grid_conjugate_gradient",
    "ccp_grid_mg_conjugate_gradient", "ccp_grid_mg_apply", "ccp_grid_mg_level",
    "ccp_grid_mg_set_hierarchy", "ccp_grid_mg_get_hierarchy", "ccp_grid_mg_set_precision", "ccp_grid_mg_get_precision",
    "ccp_grid_mg_set_channels", "ccp_grid_mg_get_channels", "ccp_debug_mgb_tile_lds",
    "ccp_grid_mg_set_smoother", "ccp_grid_mg_get_smoother",
    "ccp_grid_mg_set_nullspace", "ccp_grid_mg_get_nullspace", "ccp_grid_mg_nullspace_info",
    "ccp_grid_residual_norm2", "ccp_grid_abs_sum", "ccp_grid_assemble_rhs", "ccp_grid_assemble_from_images", "ccp_grid_store_u8",
    "ccp_grid_set_x_u8", "ccp_grid_assemble_region_rhs", "ccp_grid_assemble_clone", "ccp_grid_store_u8_composite",
    "ccp_grid_last_timing", "ccp_grid_region_begin", "ccp_grid_region_end",
    "ccp_grid_set_b_device", "ccp_grid_set_x_device", "ccp_grid_get_x_device", "ccp_grid_get_b_device",
    "ccp_grid_assemble_rhs_device", "ccp_grid_assemble_from_images_device", "ccp_grid_store_u8_device", "ccp_grid_set_x_u8_device",
    "ccp_grid_assemble_region_rhs_device", "ccp_grid_assemble_clone_device", "ccp_grid_store_u8_composite_device",
    "ccp_grid_set_weights_host", "ccp_grid_set_weights_device", "ccp_grid_assemble_weighted_rhs", "ccp_grid_assemble_weighted_rhs_device",
    "ccp_grid_set_weights_constrained_host", "ccp_grid_set_weights_constrained_device", "ccp_grid_assemble_constrained_rhs",
    "ccp_grid_assemble_constrained_rhs_device", "ccp_grid_constraint_info",
    "ccp_grid_adjoint_begin_device", "ccp_grid_weighted_adjoint_device",
    "ccp_grid_set_weights_per_channel_device", "ccp_grid_operator_channels", "ccp_grid_mg_level_channel",
    "ccp_grid_constraint_info_channel",
    "ccp_grid_mg_prepare", "ccp_grid_mg_conjugate_gradient_enqueue", "ccp_grid_mg_conjugate_gradient_enqueue_relative",
    "ccp_grid_refresh_weights_device", "ccp_grid_operator_status",
    "ccp_grid_reserve_constraints", "ccp_grid_refresh_constrained_device", "ccp_grid_reweight_device",
    "ccp_grid_reweight_robust_device", "ccp_grid_reweight_adjoint_device", "ccp_grid_irls_adjoint_step_device",
    "ccp_grid_set_mask_device", "ccp_mask_erode_cross_device", "ccp_panorama_begin_device", "ccp_panorama_add_device",
    "ccp_panorama_finish_device",
    "ccp_comm_probe", "ccp_comm_unique_id", "ccp_comm_create", "ccp_comm_destroy", "ccp_comm_info", "ccp_comm_all_reduce_sum", "ccp_comm_all_reduce_max",
    "ccp_grid_attach_comm", "ccp_grid_set_overlap", "ccp_grid_exchange_halos", "ccp_grid_sweep_rowblocked",
    "ccp_grid_gauss_seidel_rowblocked", "ccp_grid_conjugate_gradient_rowblocked", "ccp_grid_residual_norm2_global", "ccp_grid_comm_stats",
    "ccp_grid_mg_conjugate_gradient_rowblocked", "ccp_grid_mg_apply_rowblocked", "ccp_grid_mg_rowblock_info",
)


class CcpError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: status {status} ({status_string(status)})")


class Report(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32),
                ("last_l1_step", C.c_double), ("seconds", C.c_double)]


class GridDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("row_begin", C.c_int32), ("row_count", C.c_int32), ("ghost", C.c_int32),
                ("device", C.c_int32), ("flags", C.c_int32)]


class GridLayout(C.Structure):
    _fields_ = [("x_dev", C.c_void_p), ("b_dev", C.c_void_p), ("pitch", C.c_int64),
                ("local_rows", C.c_int32), ("ghost_top", C.c_int32), ("ghost_bottom", C.c_int32),
                ("channels", C.c_int32)]


DTYPE_U8, DTYPE_F32, DTYPE_F64 = 1, 2, 3


class DeviceArray(C.Structure):
    """ccp_device_array: a strided view of device memory, strides in elements."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("stride_n", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("stride_c", C.c_int64)]


ADJOINT_INPUTS = ("u", "grad_x", "gx", "gy", "f", "wx", "wy", "lambda", "fixed")
ADJOINT_OUTPUTS = ("g_wx", "g_wy", "g_lambda", "g_gx", "g_gy", "g_f", "g_values")


class AdjointInputs(C.Structure):
    """ccp_adjoint_inputs: one ccp_device_array pointer per input of the gradient pass (NULL: absent)."""
    _fields_ = [(n, C.POINTER(DeviceArray)) for n in ADJOINT_INPUTS]


class AdjointOutputs(C.Structure):
    """ccp_adjoint_outputs: one ccp_device_array pointer per gradient (NULL: not asked for)."""
    _fields_ = [(n, C.POINTER(DeviceArray)) for n in ADJOINT_OUTPUTS]


# ccp_grid_reweight_device (ccp_gs.h, "Reweighting a weighted operator from the solution"): names -> CCP_REWEIGHT_*
REWEIGHT_PENALTIES = {"charbonnier": 0, "huber": 1, "reciprocal": 2}
REWEIGHT_COUPLINGS = {"edge": 0, "pixel": 1}
REWEIGHT_VIEWS = ("u", "gx", "gy", "base_wx", "base_wy", "lambda", "out_wx", "out_wy")


def reweight_ids(penalty, coupling):
    """(CCP_REWEIGHT_* penalty, coupling) of "charbonnier" | "huber" | "reciprocal" and "edge" | "pixel": ValueError otherwise."""
    if penalty not in REWEIGHT_PENALTIES:
        raise ValueError(f"penalty must be one of {sorted(REWEIGHT_PENALTIES)}, not {penalty!r}")
    if coupling not in REWEIGHT_COUPLINGS:
        raise ValueError(f"coupling must be one of {sorted(REWEIGHT_COUPLINGS)}, not {coupling!r}")
    return REWEIGHT_PENALTIES[penalty], REWEIGHT_COUPLINGS[coupling]


class Reweight(C.Structure):
    """ccp_reweight: the penalty, the coupling, scale, epsilon and one ccp_device_array pointer per view (NULL: absent)."""
    _fields_ = [("penalty", C.c_int32), ("coupling", C.c_int32), ("scale", C.c_double), ("epsilon", C.c_double)] + \
               [(n, C.POINTER(DeviceArray)) for n in REWEIGHT_VIEWS]


# ccp_grid_reweight_robust_device (ccp_gs.h, "Robust data term"): its penalties are ccp_grid_reweight_device's and
# "quadratic" (phi = 1.0: the term is not reweighted), which reweight_ids keeps refusing for the older call
ROBUST_PENALTIES = dict(REWEIGHT_PENALTIES, quadratic=3)


def robust_ids(penalty, coupling, data_penalty):
    """(CCP_REWEIGHT_* edge penalty, coupling, data penalty) of the names ccp_grid_reweight_robust_device takes: ValueError otherwise."""
    for what, name in (("penalty", penalty), ("data_penalty", data_penalty)):
        if name not in ROBUST_PENALTIES:
            raise ValueError(f"{what} must be one of {sorted(ROBUST_PENALTIES)}, not {name!r}")
    if coupling not in REWEIGHT_COUPLINGS:
        raise ValueError(f"coupling must be one of {sorted(REWEIGHT_COUPLINGS)}, not {coupling!r}")
    return ROBUST_PENALTIES[penalty], REWEIGHT_COUPLINGS[coupling], ROBUST_PENALTIES[data_penalty]


class ReweightData(C.Structure):
    """ccp_reweight_data: the data penalty, scale, epsilon, f and the output for the lambda formed (NULL: absent)."""
    _fields_ = [("penalty", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double), ("epsilon", C.c_double),
                ("f", C.POINTER(DeviceArray)), ("out_lambda", C.POINTER(DeviceArray))]


# ccp_grid_reweight_adjoint_device (ccp_gs.h, "Backpropagating through a reweight")
REWEIGHT_GRADS_IN = ("grad_wx", "grad_wy", "grad_lambda")
REWEIGHT_GRADS_OUT = ("g_u", "g_gx", "g_gy", "g_f", "g_base_wx", "g_base_wy", "g_lambda")


class ReweightGrads(C.Structure):
    """ccp_reweight_grads: one ccp_device_array pointer per upstream gradient (NULL: 0) and per output (NULL: not computed)."""
    _fields_ = [(n, C.POINTER(DeviceArray)) for n in REWEIGHT_GRADS_IN + REWEIGHT_GRADS_OUT]


class IrlsAdjointStep(C.Structure):
    """ccp_irls_adjoint_step (ccp_gs.h, "Differentiating IRLS at its fixed point"): G, the mask of fixed pixels, the report."""
    _fields_ = [(n, C.POINTER(DeviceArray)) for n in ("grad_x", "fixed", "report")]


class PanoramaState(C.Structure):
    """ccp_panorama_state: the extents and the four views (dx, dy, raw, mask) of a panorama merge."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.POINTER(DeviceArray)) for n in ("dx", "dy", "raw", "mask")]


_lib: Optional[C.CDLL] = None

# Live handles, closed in dependency order (grids before the communicators they are attached to, both
# before the HIP / RCCL runtimes unload) if the program exits without closing them itself.
_live_grids: "weakref.WeakSet" = weakref.WeakSet()
_live_comms: "weakref.WeakSet" = weakref.WeakSet()


def _close_all_at_exit() -> None:
    for pool in (_live_grids, _live_comms):
        for h in list(pool):
            try:
                h.close()
            except Exception:
                pass


atexit.register(_close_all_at_exit)


def _share_rccl_with_torch() -> None:
    """The same for RCCL, which libccp_gs.so binds at run time by soname (ccp_comm.hpp): inside a Python
    process the HIP runtime is torch's, so the collective library must be the one torch ships with it.
    Importing torch (where it is installed) before the first communicator call loads that copy in torch's
    own order; the soname lookup inside the library then finds it.  (Round 2 saw a process that bound torch's
    librccl.so by hand and imported torch LATER abort at exit; root-caused in round 3 to RTLD_GLOBAL symbol
    interposition between librocm_smi64 and libamd_smi and fixed in csrc/ccp_comm.hip — that order is a
    regression test now, tests/test_gpu_rccl.py — so this import is about sharing ONE runtime, not about the exit.)"""
    import importlib.util
    if "torch" in sys.modules or os.environ.get("CCP_GS_NO_TORCH_HIP") or os.environ.get("CCP_GS_RCCL_LIB"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).  Whichever
    copy is loaded first serves the whole process; if ours pulled in /opt/rocm's first, a later
    `import torch` would run on a runtime it was not built for and report no GPU.  So when torch
    is installed but not imported yet, load ITS runtime first (no torch import, no GPU init)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("CCP_GS_NO_TORCH_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def load() -> C.CDLL:
    """dlopen libccp_gs.so; raises FileNotFoundError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `make -C coursecomputationalphotography_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.ccp_status_string.restype = C.c_char_p
    L.ccp_status_string.argtypes = [C.c_int]
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.ccp_csr_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.ccp_csr_destroy.argtypes = [vp]
    L.ccp_csr_upload.argtypes = [vp, i32, i32, i64, vp, vp, vp, vp]
    L.ccp_csr_upload_rows.argtypes = [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp, i32]
    L.ccp_csr_rows_info.argtypes = [vp] + [C.POINTER(i32)] * 5 + [C.POINTER(i64)] * 2
    L.ccp_csr_set_colouring.argtypes = [vp, vp, i32]
    L.ccp_csr_get_colouring.argtypes = [vp, vp, C.POINTER(i32)]
    L.ccp_csr_insert.argtypes = [vp, i32, i32, dbl]
    L.ccp_csr_insert_many.argtypes = [vp, i64, vp, vp, vp]
    L.ccp_csr_last_path.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.ccp_csr_edit_stats.argtypes = [vp] + [C.POINTER(i64)] * 5
    L.ccp_csr_device_footprint.argtypes = [vp] + [C.POINTER(i64)] * 2
    L.ccp_csr_gauss_seidel.argtypes = [vp, vp, vp, vp, dbl, i32, i32, i32, C.POINTER(Report)]
    L.ccp_csr_conjugate_gradient.argtypes = [vp, vp, vp, vp, dbl, i32, C.POINTER(Report)]
    L.ccp_csr_conjugate_gradient_jacobi.argtypes = [vp, vp, vp, dbl, i32, C.POINTER(Report)]
    L.ccp_grid_conjugate_gradient.argtypes = [vp, dbl, i32, C.POINTER(Report)]
    L.ccp_grid_mg_conjugate_gradient.argtypes = [vp, dbl, i32, i32, C.POINTER(Report)]
    L.ccp_grid_mg_apply.argtypes = [vp, i32]
    L.ccp_grid_mg_prepare.argtypes = [vp, i32]
    L.ccp_grid_mg_conjugate_gradient_enqueue.argtypes = [vp, dbl, i32, i32, C.POINTER(DeviceArray)]
    L.ccp_grid_mg_conjugate_gradient_enqueue_relative.argtypes = [vp, dbl, dbl, i32, i32, C.POINTER(DeviceArray)]
    L.ccp_grid_mg_level.argtypes = [vp, i32] + [C.POINTER(i32)] * 3 + [vp] * 3
    for option in MG_OPTIONS:
        getattr(L, f"ccp_grid_mg_set_{option}").argtypes = [vp, i32]
        getattr(L, f"ccp_grid_mg_get_{option}").argtypes = [vp, C.POINTER(i32)]
    L.ccp_grid_mg_nullspace_info.argtypes = [vp, i32, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int64)]
    L.ccp_debug_mgb_tile_lds.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ccp_csr_apply_to_vector.argtypes = [vp, vp, vp]
    L.ccp_csr_residual_norm2.argtypes = [vp, vp, vp, C.POINTER(dbl), C.POINTER(dbl)]
    L.ccp_grid_create.argtypes = [C.POINTER(GridDesc), C.POINTER(vp)]
    L.ccp_grid_destroy.argtypes = [vp]
    L.ccp_grid_get_layout.argtypes = [vp, C.POINTER(GridLayout)]
    L.ccp_grid_set_stream.argtypes = [vp, vp]
    L.ccp_grid_synchronize.argtypes = [vp]
    for name in ("ccp_grid_set_b_host", "ccp_grid_set_x_host", "ccp_grid_get_x_host", "ccp_grid_get_b_host"):
        getattr(L, name).argtypes = [vp, i32, vp, i32, i32]
    L.ccp_grid_set_mask_host.argtypes = [vp, vp, i64]
    L.ccp_grid_fill_x.argtypes = [vp, dbl]
    L.ccp_grid_b_from_x.argtypes = [vp]
    L.ccp_grid_randomize_x.argtypes = [vp, C.c_uint64, dbl, dbl]
    L.ccp_grid_sweep.argtypes = [vp, i32]
    L.ccp_grid_sweep_edges_first.argtypes = [vp, i32, i32]
    L.ccp_grid_stream_wait_edges.argtypes = [vp, vp]
    L.ccp_grid_sweep_l1.argtypes = [vp, vp]
    L.ccp_grid_tune.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_float)]
    L.ccp_grid_set_fused.argtypes = [vp, i32]
    L.ccp_grid_set_tiling.argtypes = [vp, i32, i32]
    L.ccp_grid_get_tiling.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ccp_grid_halo_refreshed.argtypes = [vp]
    L.ccp_grid_gauss_seidel.argtypes = [vp, dbl, i32, i32, C.POINTER(Report)]
    L.ccp_grid_gauss_seidel_lexicographic.argtypes = [vp, dbl, i32, i32, C.POINTER(Report)]
    L.ccp_grid_residual_norm2.argtypes = [vp, vp]
    L.ccp_grid_abs_sum.argtypes = [vp, vp]
    L.ccp_grid_assemble_rhs.argtypes = [vp, vp, vp, i64, vp]
    L.ccp_grid_assemble_from_images.argtypes = [vp, vp, i32, i64, vp, i64, i32]
    L.ccp_grid_store_u8.argtypes = [vp, vp, i64]
    L.ccp_grid_set_x_u8.argtypes = [vp, vp, i64]
    L.ccp_grid_assemble_region_rhs.argtypes = [vp, vp, vp, i64, vp, i64, i32]
    L.ccp_grid_assemble_clone.argtypes = [vp, vp, i64, vp, i64, i32, i32]
    L.ccp_grid_store_u8_composite.argtypes = [vp, vp, i64, vp, i64]
    da = C.POINTER(DeviceArray)
    for name in ("ccp_grid_set_b_device", "ccp_grid_set_x_device", "ccp_grid_get_x_device", "ccp_grid_get_b_device"):
        getattr(L, name).argtypes = [vp, da, i32, i32]
    L.ccp_grid_assemble_rhs_device.argtypes = [vp, da, da, vp]
    L.ccp_grid_assemble_from_images_device.argtypes = [vp, da, i32, da, i32]
    L.ccp_grid_store_u8_device.argtypes = [vp, da]
    L.ccp_grid_set_x_u8_device.argtypes = [vp, da]
    L.ccp_grid_assemble_region_rhs_device.argtypes = [vp, da, da, da, i32]
    L.ccp_grid_assemble_clone_device.argtypes = [vp, da, da, i32, i32]
    L.ccp_grid_store_u8_composite_device.argtypes = [vp, da, da]
    L.ccp_grid_set_weights_host.argtypes = [vp, vp, vp, vp, i64]
    L.ccp_grid_set_weights_device.argtypes = [vp, da, da, da]
    L.ccp_grid_assemble_weighted_rhs.argtypes = [vp, vp, vp, i64, vp, i64, i32]
    L.ccp_grid_assemble_weighted_rhs_device.argtypes = [vp, da, da, da, i32]
    L.ccp_grid_set_weights_constrained_host.argtypes = [vp, vp, vp, vp, i64, vp, i64]
    L.ccp_grid_set_weights_constrained_device.argtypes = [vp, da, da, da, da]
    L.ccp_grid_assemble_constrained_rhs.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, i32]
    L.ccp_grid_assemble_constrained_rhs_device.argtypes = [vp, da, da, da, da, i32]
    L.ccp_grid_constraint_info.argtypes = [vp, vp, vp, vp]
    L.ccp_grid_set_weights_per_channel_device.argtypes = [vp, vp, vp, vp, vp]
    L.ccp_grid_operator_channels.argtypes = [vp, C.POINTER(i32)]
    L.ccp_grid_refresh_weights_device.argtypes = [vp, vp, vp, vp]
    L.ccp_grid_operator_status.argtypes = [vp, C.POINTER(i32)]
    L.ccp_grid_reserve_constraints.argtypes = [vp, i32]
    L.ccp_grid_refresh_constrained_device.argtypes = [vp, vp, vp, vp, vp]
    L.ccp_grid_reweight_device.argtypes = [vp, C.POINTER(Reweight)]
    L.ccp_grid_reweight_robust_device.argtypes = [vp, C.POINTER(Reweight), C.POINTER(ReweightData)]
    L.ccp_grid_reweight_adjoint_device.argtypes = [vp, C.POINTER(Reweight), C.POINTER(ReweightData), C.POINTER(ReweightGrads)]
    L.ccp_grid_irls_adjoint_step_device.argtypes = [vp, C.POINTER(Reweight), C.POINTER(ReweightData), C.POINTER(IrlsAdjointStep)]
    L.ccp_grid_mg_level_channel.argtypes = [vp, i32, i32] + [C.POINTER(i32)] * 3 + [vp] * 3
    L.ccp_grid_constraint_info_channel.argtypes = [vp, i32, vp, vp, vp]
    L.ccp_grid_adjoint_begin_device.argtypes = [vp, da]
    L.ccp_grid_weighted_adjoint_device.argtypes = [vp, C.POINTER(AdjointInputs), C.POINTER(AdjointOutputs)]
    L.ccp_grid_set_mask_device.argtypes = [vp, da]
    ps = C.POINTER(PanoramaState)
    L.ccp_mask_erode_cross_device.argtypes = [i32, vp, i32, i32, da, da, i32]
    L.ccp_panorama_begin_device.argtypes = [i32, vp, ps, da, da]
    L.ccp_panorama_add_device.argtypes = [i32, vp, ps, da, da, da]
    L.ccp_panorama_finish_device.argtypes = [i32, vp, ps]
    L.ccp_grid_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i32)]
    L.ccp_grid_region_begin.argtypes = [vp]
    L.ccp_grid_region_end.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i64), C.POINTER(i64)]
    L.ccp_comm_probe.argtypes = [i32]
    L.ccp_comm_unique_id.argtypes = [vp]
    L.ccp_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.ccp_comm_destroy.argtypes = [vp]
    L.ccp_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ccp_comm_all_reduce_sum.argtypes = [vp, vp, i32]
    L.ccp_comm_all_reduce_max.argtypes = [vp, vp, i32]
    L.ccp_grid_attach_comm.argtypes = [vp, vp]
    L.ccp_grid_set_overlap.argtypes = [vp, i32]
    L.ccp_grid_exchange_halos.argtypes = [vp]
    L.ccp_grid_sweep_rowblocked.argtypes = [vp, i32]
    L.ccp_grid_gauss_seidel_rowblocked.argtypes = [vp, dbl, i32, i32, C.POINTER(Report)]
    L.ccp_grid_conjugate_gradient_rowblocked.argtypes = [vp, dbl, i32, C.POINTER(Report)]
    L.ccp_grid_mg_conjugate_gradient_rowblocked.argtypes = [vp, dbl, i32, i32, C.POINTER(Report)]
    L.ccp_grid_mg_apply_rowblocked.argtypes = [vp, i32]
    L.ccp_grid_mg_rowblock_info.argtypes = [vp] + [C.POINTER(i32)] * 4
    L.ccp_grid_residual_norm2_global.argtypes = [vp, vp]
    L.ccp_grid_comm_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    _lib = L
    return L


def status_string(status: int) -> str:
    try:
        return load().ccp_status_string(status).decode()
    except Exception:
        return "?"


def check(status: int, what: str) -> None:
    if status != CCP_OK:
        raise CcpError(status, what)


def device_count() -> int:
    return int(load().ccp_device_count())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _refs(arrs):
    """byref of every ccp_device_array of `arrs`, None (a NULL argument) kept."""
    return [None if a is None else C.byref(a) for a in arrs]


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _no_overlap(shape, strides) -> bool:
    """No two elements of a view share an address: sorted by stride, each stride >= stride * extent of the one below
    (dimensions of extent 1 do not count)."""
    dims = sorted((s, e) for s, e in zip(strides, shape) if e > 1)
    span = 1
    for s, e in dims:
        if s < span:
            return False
        span = s * e
    return True


COMM_ID_BYTES = 128


def comm_probe(device: int = 0) -> None:
    """Raises CcpError unless this process can take part in a communicator on `device` (not collective)."""
    _share_rccl_with_torch()
    check(load().ccp_comm_probe(device), "ccp_comm_probe")


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI (rank 0 calls this and hands the bytes to the other ranks)."""
    _share_rccl_with_torch()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(load().ccp_comm_unique_id(buf), "ccp_comm_unique_id")
    return bytes(buf)


class Comm:
    """One rank of an RCCL communicator behind the C ABI (ccp_comm_*).  Creation is collective."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int = 0):
        _share_rccl_with_torch()
        self.L = load()
        self.h = C.c_void_p()
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique id must be COMM_ID_BYTES long")
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(self.L.ccp_comm_create(buf, rank, world, device, C.byref(self.h)), "ccp_comm_create")
        self.rank, self.world, self.device = rank, world, device
        _live_comms.add(self)

    def info(self):
        r, w, d, v = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.ccp_comm_info(self.h, C.byref(r), C.byref(w), C.byref(d), C.byref(v)), "ccp_comm_info")
        return {"rank": r.value, "world": w.value, "device": d.value, "rccl_version": v.value}

    def all_reduce_sum(self, values) -> np.ndarray:
        a = _f64(values).copy()
        check(self.L.ccp_comm_all_reduce_sum(self.h, _ptr(a), a.size), "ccp_comm_all_reduce_sum")
        return a

    def all_reduce_max(self, values) -> np.ndarray:
        a = _f64(values).copy()
        check(self.L.ccp_comm_all_reduce_max(self.h, _ptr(a), a.size), "ccp_comm_all_reduce_max")
        return a

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ccp_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def embed_region_host(values, col_offset, row_offset, colour):
    """ccp_csr_embed_region_host: (recognised, W, H, x[n], y[n]) — the raster-region recognition alone, on the host."""
    L = load()
    values, col_offset, row_offset, colour = _f64(values), _i32(col_offset), _i32(row_offset), _i32(colour)
    n = len(row_offset) - 1
    ok, w, h = C.c_int32(), C.c_int32(), C.c_int32()
    x, y = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    L.ccp_csr_embed_region_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(C.c_int32)] * 3 + [C.c_void_p] * 2
    check(L.ccp_csr_embed_region_host(n, _ptr(row_offset), _ptr(col_offset), _ptr(values), _ptr(colour), C.byref(ok), C.byref(w),
                                      C.byref(h), _ptr(x), _ptr(y)), "ccp_csr_embed_region_host")
    return bool(ok.value), w.value, h.value, x[:n], y[:n]


class CsrMatrix:
    """Device-resident slack-CSR matrix (ccp_csr_*)."""

    def __init__(self, device: int = 0):
        self.L = load()
        self.h = C.c_void_p()
        check(self.L.ccp_csr_create(device, C.byref(self.h)), "ccp_csr_create")
        self.n_rows = self.n_cols = 0

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ccp_csr_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def upload(self, n_rows, n_cols, values, col_offset, row_begin, row_num_nze):
        values, col_offset = _f64(values), _i32(col_offset)
        row_begin, row_num_nze = _i32(row_begin), _i32(row_num_nze)
        check(self.L.ccp_csr_upload(self.h, n_rows, n_cols, len(values), _ptr(values), _ptr(col_offset),
                                    _ptr(row_begin), _ptr(row_num_nze)), "ccp_csr_upload")
        self.n_rows, self.n_cols = n_rows, n_cols
        return self

    def upload_rows(self, comm: "Comm", first_row, n_global, values, col_offset, row_begin, row_num_nze, colour, n_colours):
        """COLLECTIVE: this handle becomes the block of rows [first_row, first_row + len(row_begin)) of an n_global-row
        matrix distributed over comm's ranks (global column indices; colour: the owned rows of a proper colouring of the
        whole matrix).  Afterwards gauss_seidel / apply_to_vector / residual_norm2 take and return the block's own rows."""
        values, col_offset = _f64(values), _i32(col_offset)
        row_begin, row_num_nze, colour = _i32(row_begin), _i32(row_num_nze), _i32(colour)
        n_rows = len(row_begin)
        check(self.L.ccp_csr_upload_rows(self.h, comm.h, first_row, n_rows, n_global, len(values), _ptr(values), _ptr(col_offset),
                                         _ptr(row_begin), _ptr(row_num_nze), _ptr(colour), n_colours), "ccp_csr_upload_rows")
        self.n_rows = self.n_cols = n_rows
        return self

    def rows_info(self):
        a = [C.c_int32() for _ in range(5)]
        b = [C.c_int64() for _ in range(2)]
        check(self.L.ccp_csr_rows_info(self.h, *[C.byref(t) for t in a + b]), "ccp_csr_rows_info")
        return dict(zip(("first_row", "n_rows", "n_ghost", "n_peers", "edge_slices", "values_sent", "exchanges"), (t.value for t in a + b)))

    def upload_compressed(self, values, col_offset, row_offset, n_cols=None):
        """Compressed CSR (n+1 offsets) -> the slack arrays with zero slack."""
        row_offset = _i32(row_offset)
        n = len(row_offset) - 1
        return self.upload(n, n if n_cols is None else n_cols, values, col_offset, row_offset[:-1],
                           np.diff(row_offset))

    def set_colouring(self, colour, n_colours=None):
        if colour is None:
            check(self.L.ccp_csr_set_colouring(self.h, None, 0), "ccp_csr_set_colouring")
            return self
        colour = _i32(colour)
        nc = int(colour.max()) + 1 if n_colours is None else n_colours
        check(self.L.ccp_csr_set_colouring(self.h, _ptr(colour), nc), "ccp_csr_set_colouring")
        return self

    def insert(self, val: float, row: int, col: int):
        """SparseMatrix::insert(val, row, col) on the uploaded matrix (applied on the device incrementally)."""
        check(self.L.ccp_csr_insert(self.h, row, col, float(val)), "ccp_csr_insert")

    def last_path(self) -> str:
        """Kernels of the last gauss_seidel: "sliced ELL", "Poisson grid WxH" or "region grid WxH" (canvas)."""
        p, w, h, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        check(self.L.ccp_csr_last_path(self.h, C.byref(p), C.byref(w), C.byref(h), C.byref(n)), "ccp_csr_last_path")
        self.last_sweep_launches = n.value
        return {0: "sliced ELL", 1: f"Poisson grid {w.value}x{h.value}", 2: f"region grid {w.value}x{h.value}"}[p.value]

    def insert_many(self, vals, rows, cols):
        vals, rows, cols = _f64(vals), _i32(rows), _i32(cols)
        check(self.L.ccp_csr_insert_many(self.h, len(vals), _ptr(rows), _ptr(cols), _ptr(vals)), "ccp_csr_insert_many")

    def edit_stats(self):
        v = [C.c_int64() for _ in range(5)]
        check(self.L.ccp_csr_edit_stats(self.h, *[C.byref(t) for t in v]), "ccp_csr_edit_stats")
        return dict(zip(("edits", "image_uploads", "rows_patched", "slices_relocated", "image_rebuilds"), (t.value for t in v)))

    def device_footprint(self):
        """(device bytes held for a copy of the stored matrix, uploads whose background copy was skipped for lack of room)."""
        v = [C.c_int64() for _ in range(2)]
        check(self.L.ccp_csr_device_footprint(self.h, *[C.byref(t) for t in v]), "ccp_csr_device_footprint")
        return v[0].value, v[1].value

    def get_colouring(self):
        """(colour[n_rows], n_colours) the multi-colour sweep uses (caller's or the library's greedy one)."""
        colour = np.empty(max(self.n_rows, 1), dtype=np.int32)
        nc = C.c_int32()
        check(self.L.ccp_csr_get_colouring(self.h, _ptr(colour), C.byref(nc)), "ccp_csr_get_colouring")
        return colour[:self.n_rows], nc.value

    def gauss_seidel(self, b, epsilon=1e-6, max_iteration=1000, x0=None, check_every=1,
                     ordering=ORDER_MULTICOLOUR, out=None):
        """out: a float64 array of n_cols entries to receive x (a buffer that is used again travels at the PCIe rate: the
        HIP runtime registers a host buffer at its first use — 54 GB/s against 10-17 GB/s into fresh pages)."""
        b = _f64(b)
        x0a = None if x0 is None else _f64(x0)
        if out is not None and (out.dtype != np.float64 or out.size != self.n_cols or not out.flags.c_contiguous):
            raise ValueError("out must be a contiguous float64 array of n_cols entries")
        x = np.empty(self.n_cols, dtype=np.float64) if out is None else out
        rep = Report()
        check(self.L.ccp_csr_gauss_seidel(self.h, _ptr(b), _ptr(x0a), _ptr(x), epsilon, max_iteration,
                                          check_every, ordering, C.byref(rep)), "ccp_csr_gauss_seidel")
        return x, rep

    def conjugate_gradient(self, b, epsilon=1e-16, max_iteration=1000, init=None):
        b = _f64(b)
        ia = None if init is None else _f64(init)
        x = np.empty(self.n_cols, dtype=np.float64)
        rep = Report()
        check(self.L.ccp_csr_conjugate_gradient(self.h, _ptr(b), _ptr(ia), _ptr(x), epsilon, max_iteration,
                                                C.byref(rep)), "ccp_csr_conjugate_gradient")
        return x, rep

    def conjugate_gradient_jacobi(self, b, epsilon=1e-16, max_iteration=180):
        """SparseMatrix::conjugateGradientEigen: Jacobi-preconditioned, from x0 = 0."""
        b = _f64(b)
        x = np.empty(self.n_cols, dtype=np.float64)
        rep = Report()
        check(self.L.ccp_csr_conjugate_gradient_jacobi(self.h, _ptr(b), _ptr(x), epsilon, max_iteration, C.byref(rep)),
              "ccp_csr_conjugate_gradient_jacobi")
        return x, rep

    def apply_to_vector(self, v):
        v = _f64(v)
        out = np.empty(self.n_rows, dtype=np.float64)
        check(self.L.ccp_csr_apply_to_vector(self.h, _ptr(v), _ptr(out)), "ccp_csr_apply_to_vector")
        return out

    def residual_norm2(self, b, x):
        b, x = _f64(b), _f64(x)
        rr, bb = C.c_double(), C.c_double()
        check(self.L.ccp_csr_residual_norm2(self.h, _ptr(b), _ptr(x), C.byref(rr), C.byref(bb)),
              "ccp_csr_residual_norm2")
        return rr.value, bb.value


class Grid:
    """Structured Poisson grid block (ccp_grid_*)."""

    def __init__(self, width, height, channels=1, row_begin=0, row_count=None, ghost=0, device=0, mask=None, weighted=False):
        """mask: H x W array (non-zero = unknown) makes this a Dirichlet-mask grid (CCP_GRID_DIRICHLET_MASK); weighted:
        a weighted grid (CCP_GRID_WEIGHTED: set_weights, then assemble_weighted_rhs; single blocks, no mask)."""
        self.L = load()
        self.h = C.c_void_p()
        row_count = height if row_count is None else row_count
        flags = (0 if mask is None else GRID_DIRICHLET_MASK) | (GRID_WEIGHTED if weighted else 0)
        self.desc = GridDesc(width, height, channels, row_begin, row_count, ghost, device, flags)
        check(self.L.ccp_grid_create(C.byref(self.desc), C.byref(self.h)), "ccp_grid_create")
        self.layout = GridLayout()
        check(self.L.ccp_grid_get_layout(self.h, C.byref(self.layout)), "ccp_grid_get_layout")
        self.W, self.H, self.C = width, height, channels
        self.row_begin, self.row_count = row_begin, row_count
        self.first_local_row = row_begin - self.layout.ghost_top       # image row of local row 0
        self.local_rows = self.layout.local_rows
        self._comm = None
        self.stream_handle = 0                                   # the null stream until set_stream says otherwise
        _live_grids.add(self)
        if mask is not None:
            self.set_mask(mask)

    def set_mask(self, mask):
        """The region from an H x W host array, or from a CUDA tensor (set_mask_tensor: read on the device)."""
        if getattr(mask, "is_cuda", False):
            return self.set_mask_tensor(mask)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != (self.H, self.W):
            raise ValueError("mask must be H x W")
        check(self.L.ccp_grid_set_mask_host(self.h, _ptr(mask), mask.strides[0]), "ccp_grid_set_mask_host")

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ccp_grid_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int):
        check(self.L.ccp_grid_set_stream(self.h, C.c_void_p(stream_handle)), "ccp_grid_set_stream")
        self.stream_handle = int(stream_handle or 0)

    def synchronize(self):
        check(self.L.ccp_grid_synchronize(self.h), "ccp_grid_synchronize")

    def _rows(self, first_row, n_rows):
        if first_row is None:
            first_row = self.first_local_row
        if n_rows is None:
            n_rows = self.local_rows - (first_row - self.first_local_row)
        return first_row, n_rows

    def set_b(self, rows, channel=0, first_row=None):
        rows = _f64(rows).reshape(-1, self.W)
        first_row, _ = self._rows(first_row, None)
        check(self.L.ccp_grid_set_b_host(self.h, channel, _ptr(rows), first_row, rows.shape[0]), "ccp_grid_set_b_host")

    def set_x(self, rows, channel=0, first_row=None):
        rows = _f64(rows).reshape(-1, self.W)
        first_row, _ = self._rows(first_row, None)
        check(self.L.ccp_grid_set_x_host(self.h, channel, _ptr(rows), first_row, rows.shape[0]), "ccp_grid_set_x_host")

    def get_x(self, channel=0, first_row=None, n_rows=None) -> np.ndarray:
        first_row, n_rows = self._rows(first_row, n_rows)
        out = np.empty((n_rows, self.W), dtype=np.float64)
        check(self.L.ccp_grid_get_x_host(self.h, channel, _ptr(out), first_row, n_rows), "ccp_grid_get_x_host")
        return out

    def get_b(self, channel=0, first_row=None, n_rows=None) -> np.ndarray:
        first_row, n_rows = self._rows(first_row, n_rows)
        out = np.empty((n_rows, self.W), dtype=np.float64)
        check(self.L.ccp_grid_get_b_host(self.h, channel, _ptr(out), first_row, n_rows), "ccp_grid_get_b_host")
        return out

    def get_x_owned(self, channel=0) -> np.ndarray:
        return self.get_x(channel, self.row_begin, self.row_count)

    def fill_x(self, value=1.0):
        check(self.L.ccp_grid_fill_x(self.h, value), "ccp_grid_fill_x")

    def randomize_x(self, seed, lo=0.0, hi=255.0):
        check(self.L.ccp_grid_randomize_x(self.h, seed, lo, hi), "ccp_grid_randomize_x")

    def b_from_x(self):
        check(self.L.ccp_grid_b_from_x(self.h), "ccp_grid_b_from_x")

    def sweep(self, iterations):
        check(self.L.ccp_grid_sweep(self.h, iterations), "ccp_grid_sweep")

    def sweep_edges_first(self, iterations, edge_rows):
        """sweep(), with the rows a neighbour block needs finished first in the last pass."""
        check(self.L.ccp_grid_sweep_edges_first(self.h, iterations, edge_rows), "ccp_grid_sweep_edges_first")

    def stream_wait_edges(self, stream_handle: int):
        check(self.L.ccp_grid_stream_wait_edges(self.h, C.c_void_p(stream_handle)), "ccp_grid_stream_wait_edges")

    def tune(self, max_t: int = 8):
        """Time the (depth, rows-per-chunk) candidates on this shape; returns (T, rows, ms/iter)."""
        t, r, ms = C.c_int32(), C.c_int32(), C.c_float()
        check(self.L.ccp_grid_tune(self.h, max_t, C.byref(t), C.byref(r), C.byref(ms)), "ccp_grid_tune")
        return t.value, r.value, ms.value

    def set_fused(self, on: bool):
        """Temporally blocked pass (True, default) or the in-place half-sweep kernels (False)."""
        check(self.L.ccp_grid_set_fused(self.h, 1 if on else 0), "ccp_grid_set_fused")

    def set_tiling(self, max_t: int, rows_per_chunk: int):
        check(self.L.ccp_grid_set_tiling(self.h, max_t, rows_per_chunk), "ccp_grid_set_tiling")

    def get_tiling(self):
        """(max depth, rows per chunk at that depth, tuned?) of the next unchecked sweep."""
        t, r, tuned = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.ccp_grid_get_tiling(self.h, C.byref(t), C.byref(r), C.byref(tuned)), "ccp_grid_get_tiling")
        return t.value, r.value, bool(tuned.value)

    def sweep_l1(self) -> np.ndarray:
        out = np.empty(self.C, dtype=np.float64)
        check(self.L.ccp_grid_sweep_l1(self.h, _ptr(out)), "ccp_grid_sweep_l1")
        return out

    def halo_refreshed(self):
        check(self.L.ccp_grid_halo_refreshed(self.h), "ccp_grid_halo_refreshed")

    def gauss_seidel(self, epsilon=1e-6, max_iteration=1000, check_every=1):
        reps = (Report * self.C)()
        check(self.L.ccp_grid_gauss_seidel(self.h, epsilon, max_iteration, check_every, reps), "ccp_grid_gauss_seidel")
        return list(reps)

    def gauss_seidel_lexicographic(self, epsilon=1e-6, max_iteration=1000, check_every=1):
        """The reference's own sweep order (index order), bit-identical iterates; whole-image handles."""
        reps = (Report * self.C)()
        check(self.L.ccp_grid_gauss_seidel_lexicographic(self.h, epsilon, max_iteration, check_every, reps),
              "ccp_grid_gauss_seidel_lexicographic")
        return list(reps)

    def conjugate_gradient(self, epsilon=1e-16, max_iteration=1000):
        reps = (Report * self.C)()
        check(self.L.ccp_grid_conjugate_gradient(self.h, epsilon, max_iteration, reps), "ccp_grid_conjugate_gradient")
        return list(reps)

    def mg_conjugate_gradient(self, epsilon, max_iteration, smoothing_sweeps=2):
        """Multigrid-preconditioned CG from the resident x, channel by channel (one Report per channel)."""
        reps = (Report * self.C)()
        check(self.L.ccp_grid_mg_conjugate_gradient(self.h, epsilon, max_iteration, smoothing_sweeps, reps),
              "ccp_grid_mg_conjugate_gradient")
        return list(reps)

    def mg_prepare(self, sweeps=0):
        """Everything mg_conjugate_gradient would do before its first launch in the handle's present configuration -- the
        checks, the hierarchy, every allocation and one-off read-back -- with the status the solve would return (CcpError).
        May synchronise; x and b are untouched.  Needed before mg_conjugate_gradient_enqueue, with the same `sweeps`, and
        again after a call that drops what it built: the operator and mask setters, the mg_set_* mode setters."""
        check(self.L.ccp_grid_mg_prepare(self.h, sweeps), "ccp_grid_mg_prepare")

    def mg_conjugate_gradient_enqueue(self, epsilon, max_iteration, sweeps=0, report=None):
        """mg_conjugate_gradient without the host: the start-up steps and exactly `max_iteration` iterations (<= 4096; a
        channel that has stopped costs no-op launches) are enqueued on torch's current stream of the handle's device, with no
        allocation and no host synchronisation, so the call may be recorded by torch.cuda.graph.  x and the figures of the
        report equal mg_conjugate_gradient's bit for bit.  Needs mg_prepare(sweeps) (CcpError STATE otherwise).
        report: a CUDA float64 tensor of channels x 6 (any non-overlapping strides), or None; a kernel fills row ch with
        iterations, converged (0.0 / 1.0), last_l1_step, b_mean, x_mean ("constant" null-space mode; 0.0 otherwise) and
        0.0 when the stream gets there.  Returns `report`."""
        arr = self._enqueue_report(report, 6)
        ref = None if arr is None else C.byref(arr)
        self._on_stream(lambda: self.L.ccp_grid_mg_conjugate_gradient_enqueue(self.h, epsilon, max_iteration, sweeps, ref),
                        "ccp_grid_mg_conjugate_gradient_enqueue")
        return report

    def _enqueue_report(self, report, fields):
        """The view of an enqueue solve's report (a CUDA float64 tensor of channels x `fields`), or None for None."""
        if report is None:
            return None
        torch = self._torch()
        if not isinstance(report, torch.Tensor) or report.device.type != "cuda" or report.device.index != self.desc.device:
            raise ValueError(f"report must be a tensor on cuda:{self.desc.device}")
        if report.dtype != torch.float64 or tuple(report.shape) != (self.C, fields):
            raise ValueError(f"report must be a float64 tensor of {self.C} x {fields}, not {report.dtype} {tuple(report.shape)}")
        if any(s < 0 for s in report.stride()) or not _no_overlap(report.shape, report.stride()):
            raise ValueError("report is an output whose elements overlap or has a negative stride")
        return DeviceArray(report.data_ptr(), DTYPE_F64, 0, 0, report.stride(0), report.stride(1), 0)

    def mg_conjugate_gradient_enqueue_relative(self, epsilon_abs, epsilon_rel, max_iteration, sweeps=0, report=None):
        """mg_conjugate_gradient_enqueue with a stop test relative to |b| that the device forms: channel c stops when
        sqrt(r'r) < max(epsilon_abs, epsilon_rel * |b_c|) or the residual is exactly 0, |b_c| summed inside the init pass that
        reads b anyway (in "constant" null-space mode: |b_c - mean(b_c)|).  The threshold lives in device memory, so a
        recorded solve follows each replay's right-hand side.  epsilon_rel = 0 is mg_conjugate_gradient_enqueue at
        epsilon_abs, bit for bit.  Negative, NaN or infinite tolerances: CcpError BAD_ARG.  Needs mg_prepare(sweeps).
        report: a CUDA float64 tensor of channels x 8, or None: the six fields of mg_conjugate_gradient_enqueue's report,
        then |b_c| and the threshold channel c stopped against.  Returns `report`."""
        arr = self._enqueue_report(report, 8)
        ref = None if arr is None else C.byref(arr)
        self._on_stream(lambda: self.L.ccp_grid_mg_conjugate_gradient_enqueue_relative(self.h, epsilon_abs, epsilon_rel, max_iteration, sweeps, ref),
                        "ccp_grid_mg_conjugate_gradient_enqueue_relative")
        return report

    def mg_apply(self, smoothing_sweeps=2):
        """x := M^-1 b (one V-cycle per channel; diagnostic)."""
        check(self.L.ccp_grid_mg_apply(self.h, smoothing_sweeps), "ccp_grid_mg_apply")

    def _mg_set(self, option, value):
        name = f"ccp_grid_mg_set_{option}"
        check(getattr(self.L, name)(self.h, _mg_value(option, value)), name)

    def _mg_get(self, option):
        value, name = C.c_int32(), f"ccp_grid_mg_get_{option}"
        check(getattr(self.L, name)(self.h, C.byref(value)), name)
        return next(n for n, v in MG_OPTIONS[option][0].items() if v == value.value)

    def mg_configure(self, *, hierarchy=None, precision=None, channels=None, smoother=None, nullspace=None):
        """mg_set_hierarchy, _precision, _channels, _smoother and _nullspace, in that order, each for an option that is
        given.  An option left at None is not set: its setter is not called, so hierarchy and nullspace, which only a
        weighted handle takes, can be left out on any other."""
        for option, value in zip(MG_OPTIONS, (hierarchy, precision, channels, smoother, nullspace)):
            if value is not None:
                self._mg_set(option, value)

    def mg_set_hierarchy(self, kind):
        """The hierarchy kind of a weighted handle: "galerkin" (the default: coarse correction scaled by 2) or "rescaled"
        (edge weights halved per level, correction unscaled: the one to choose with data weights > 0), or the integers
        MG_HIERARCHY_*.  A change drops the cached hierarchy."""
        self._mg_set("hierarchy", kind)

    @property
    def mg_hierarchy(self):
        """The handle's hierarchy kind: "galerkin" or "rescaled"."""
        return self._mg_get("hierarchy")

    def mg_set_precision(self, precision):
        """The precision of the multigrid preconditioner: "f64" (the default) or "f32" (the V-cycle in float, the outer
        PCG loop and its stop test in fp64: same answer, for weighted handles best with the "rescaled" hierarchy), or the
        integers of MG_PRECISIONS.  A change drops the cached hierarchy."""
        self._mg_set("precision", precision)

    def mg_precision(self):
        """The handle's preconditioner precision: "f64" or "f32"."""
        return self._mg_get("precision")

    def mg_set_channels(self, mode):
        """How the multigrid PCG goes through the handle's channels: "sequential" (the default: one loop per channel) or
        "batched" (one loop, every launch serves all channels; every channel gets the sequential call's bits), or the
        integers of MG_CHANNELS.  A change drops the cached PCG vectors and keeps the hierarchy."""
        self._mg_set("channels", mode)

    def mg_channels(self):
        """The handle's channel mode: "sequential" or "batched"."""
        return self._mg_get("channels")

    def mg_set_smoother(self, kind):
        """The V-cycle's smoother: "point" (the default: red-black Gauss-Seidel) or "line" (alternating zebra line
        relaxation on the levels above the tail; weighted handles, fp64, sequential channels: anything else is refused
        at the solve), or the integers of MG_SMOOTHERS.  With "line" smoothing_sweeps 0 means 1 sweep."""
        self._mg_set("smoother", kind)

    def mg_smoother(self):
        """The handle's smoother: "point" or "line"."""
        return self._mg_get("smoother")

    def mg_set_nullspace(self, kind):
        """The null space the multigrid PCG accounts for (weighted handles): "none" (the default) or "constant" -- a
        floating operator (lambda = 0 everywhere, no fixed pixel, every in-canvas edge weight > 0) is solved on the
        mean-free vectors, and x keeps the mean it came with; anything else is refused at the solve, as are batched
        channels and the line smoother on a canvas whose hierarchy has a line-smoothed level (level 0, or a coarse level
        with a side > 32) of one row or one column -- or the integers of MG_NULLSPACES."""
        self._mg_set("nullspace", kind)

    def mg_get_nullspace(self):
        """The handle's null-space mode: "none" or "constant"."""
        return self._mg_get("nullspace")

    def mg_nullspace_info(self, channel: int = 0):
        """(mean(b), mean of the returned x, W * H) of the last "constant"-mode solve of channel `channel`."""
        bm, xm, n = C.c_double(), C.c_double(), C.c_int64()
        check(self.L.ccp_grid_mg_nullspace_info(self.h, channel, C.byref(bm), C.byref(xm), C.byref(n)), "ccp_grid_mg_nullspace_info")
        return bm.value, xm.value, n.value

    def mg_levels(self, channel: int = 0):
        """The multigrid hierarchy: one (diag, w_east, w_south) triple of H_k x W_k arrays per level, level 0 first.
        channel: whose hierarchy, on a handle with one operator per channel (set_weights_per_channel_tensor)."""
        n = C.c_int32()
        check(self.L.ccp_grid_mg_level_channel(self.h, channel, 0, C.byref(n), None, None, None, None, None), "ccp_grid_mg_level_channel")
        return [self.mg_level(k, channel) for k in range(n.value)]

    def mg_level(self, level: int, channel: int = 0):
        """(diag, w_east, w_south) of one level of channel `channel`'s hierarchy."""
        w, h = C.c_int32(), C.c_int32()
        check(self.L.ccp_grid_mg_level_channel(self.h, channel, level, None, C.byref(w), C.byref(h), None, None, None),
              "ccp_grid_mg_level_channel")
        d, we, ws = (np.empty((h.value, w.value), dtype=np.float64) for _ in range(3))
        check(self.L.ccp_grid_mg_level_channel(self.h, channel, level, None, None, None, _ptr(d), _ptr(we), _ptr(ws)),
              "ccp_grid_mg_level_channel")
        return d, we, ws

    def residual_norm2(self):
        out = np.empty(2 * self.C, dtype=np.float64)
        check(self.L.ccp_grid_residual_norm2(self.h, _ptr(out)), "ccp_grid_residual_norm2")
        return out[:self.C].copy(), out[self.C:].copy()

    def abs_sum(self) -> np.ndarray:
        out = np.empty(self.C, dtype=np.float64)
        check(self.L.ccp_grid_abs_sum(self.h, _ptr(out)), "ccp_grid_abs_sum")
        return out

    def assemble_rhs(self, gx: np.ndarray, gy: np.ndarray, constraint):
        gx = np.ascontiguousarray(gx, dtype=np.float32)
        gy = np.ascontiguousarray(gy, dtype=np.float32)
        cons = _i32(constraint)
        check(self.L.ccp_grid_assemble_rhs(self.h, _ptr(gx), _ptr(gy), gx.strides[0], _ptr(cons)), "ccp_grid_assemble_rhs")

    def assemble_from_images(self, images, label: np.ndarray, init_x: bool = False):
        imgs = [np.ascontiguousarray(i, dtype=np.uint8) for i in images]
        label = np.ascontiguousarray(label, dtype=np.uint8)
        ptrs = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
        check(self.L.ccp_grid_assemble_from_images(self.h, ptrs, len(imgs), imgs[0].strides[0], _ptr(label),
                                                   label.strides[0], 1 if init_x else 0),
              "ccp_grid_assemble_from_images")

    def store_u8(self) -> np.ndarray:
        out = np.zeros((self.H, self.W, self.C), dtype=np.uint8)
        check(self.L.ccp_grid_store_u8(self.h, _ptr(out), out.strides[0]), "ccp_grid_store_u8")
        return out

    def set_x_u8(self, image: np.ndarray):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        check(self.L.ccp_grid_set_x_u8(self.h, _ptr(image), image.strides[0]), "ccp_grid_set_x_u8")

    # ---- region blends (Dirichlet-mask grids; whole-canvas H x W x channels host images) ----------------
    def _canvas_image(self, img, dtype) -> np.ndarray:
        img = np.ascontiguousarray(img, dtype=dtype)
        if img.reshape(self.H, self.W, -1).shape[2] != self.C:
            raise ValueError(f"image must be {self.H} x {self.W} x {self.C}")
        return img

    def assemble_region_rhs(self, gx, gy, canvas, init_x: bool = False):
        """b := -div(g) + the canvas values of the neighbours outside the region (0 outside); init_x: x := canvas
        inside the region.  gx, gy: float32 forward differences, canvas: u8."""
        gx, gy = self._canvas_image(gx, np.float32), self._canvas_image(gy, np.float32)
        canvas = self._canvas_image(canvas, np.uint8)
        check(self.L.ccp_grid_assemble_region_rhs(self.h, _ptr(gx), _ptr(gy), gx.strides[0], _ptr(canvas), canvas.strides[0],
                                                  1 if init_x else 0), "ccp_grid_assemble_region_rhs")

    def assemble_clone(self, source, target, mixed: bool = False, init: int = 1):
        """Seamless cloning of `source` into `target` (both u8, already on the canvas): imported (mixed False) or
        mixed gradients, boundary values from the target.  init: 0 leave x, 1 x := target, 2 x := source."""
        source, target = self._canvas_image(source, np.uint8), self._canvas_image(target, np.uint8)
        check(self.L.ccp_grid_assemble_clone(self.h, _ptr(source), source.strides[0], _ptr(target), target.strides[0],
                                             CLONE_MIXED if mixed else CLONE_IMPORT, int(init)), "ccp_grid_assemble_clone")

    def store_u8_composite(self, canvas) -> np.ndarray:
        """The clamped solution inside the region, the canvas outside; H x W x channels u8.  On a row block only the
        owned rows are filled (the others stay 0)."""
        canvas = self._canvas_image(canvas, np.uint8)
        out = np.zeros((self.H, self.W, self.C), dtype=np.uint8)
        check(self.L.ccp_grid_store_u8_composite(self.h, _ptr(canvas), canvas.strides[0], _ptr(out), out.strides[0]),
              "ccp_grid_store_u8_composite")
        return out

    # ---- device hand-off: torch tensors in, torch tensors out (ccp_grid_*_device) -----------------------------
    # Every tensor is H x W x channels (n_rows x W x channels for set/get; H x W also accepted when channels == 1),
    # any strides: interleaved, channel-planar (a C x H x W tensor .permute(1, 2, 0)), a window of a larger image or
    # an expanded (broadcast) input.  Tensors are checked here (device, dtype, shape, strides) and ValueError is raised
    # before the library is called.  Each call is enqueued on torch.cuda.current_stream(device) -- the handle's stream
    # is set to it for the call and restored afterwards -- with no host synchronisation (assemble_from_images_tensor
    # excepted), and outputs are allocated on that stream.  The caller keeps inputs unchanged until that stream has
    # passed the call, as for any torch kernel.
    def _torch(self):
        import torch
        return torch

    def _device(self):
        return self._torch().device("cuda", self.desc.device)

    def _array(self, t, name, dtypes, shape, output=False, optional=True):
        """The one check of a tensor argument, in this order: a torch tensor, on the handle's device, of one of `dtypes`,
        of extents `shape` (None: any), without a negative stride and, an output, without overlapping elements.  Returns
        its ccp_device_array (a stride the tensor lacks is 0), or None for None where `optional`."""
        if t is None and optional:
            return None
        torch = self._torch()
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.device.type != "cuda" or t.device.index != self.desc.device:
            raise ValueError(f"{name} must be on cuda:{self.desc.device}, not {t.device}")
        codes = {torch.uint8: DTYPE_U8, torch.float32: DTYPE_F32, torch.float64: DTYPE_F64}
        if t.dtype not in dtypes:
            raise ValueError(f"{name} must have dtype {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {' x '.join(str(n) for n in shape)}, not {tuple(t.shape)}")
        if any(s < 0 for s in t.stride()):
            raise ValueError(f"{name} has a negative stride")
        if output and not _no_overlap(t.shape, t.stride()):
            raise ValueError(f"{name} is an output whose elements overlap")
        return DeviceArray(t.data_ptr(), codes[t.dtype], 0, 0, *t.stride(), *[0] * (3 - t.dim()))

    def _hwc(self, t, name, dtypes, rows=None, output=False):
        """Check tensor `t` and return (ccp_device_array, t viewed as rows x W x C)."""
        if isinstance(t, self._torch().Tensor) and t.dim() == 2 and self.C == 1:
            t = t.unsqueeze(-1)
        shape = (self.H if rows is None else rows, self.W, self.C)
        return self._array(t, name, dtypes, shape, output=output, optional=False), t

    def _image(self, t, name, dtypes):
        """ccp_device_array of an optional H x W x channels tensor (None: None)."""
        return None if t is None else self._hwc(t, name, dtypes)[0]

    def _on_stream(self, fn, what):
        """Run `fn()` (a library call) on torch's current stream of this device, restoring the handle's stream."""
        torch = self._torch()
        stream = torch.cuda.current_stream(self._device()).cuda_stream
        prev = self.stream_handle
        self.set_stream(stream)
        try:
            check(fn(), what)
        finally:
            self.set_stream(prev)

    def _set_tensor(self, which, t, first_row):
        torch = self._torch()
        first_row = self.first_local_row if first_row is None else first_row
        n = t.shape[0] if hasattr(t, "shape") and len(t.shape) else 0
        arr, _ = self._hwc(t, "rows", (torch.float32, torch.float64), rows=n)
        fn = getattr(self.L, f"ccp_grid_set_{which}_device")
        self._on_stream(lambda: fn(self.h, C.byref(arr), first_row, n), f"ccp_grid_set_{which}_device")

    def _get_tensor(self, which, out, dtype, first_row, n_rows):
        torch = self._torch()
        first_row, n_rows = self._rows(first_row, n_rows)
        if out is None:
            with torch.cuda.device(self._device()):
                out = torch.empty((n_rows, self.W, self.C), dtype=dtype, device=self._device())
        arr, _ = self._hwc(out, "out", (torch.float32, torch.float64), rows=n_rows, output=True)
        fn = getattr(self.L, f"ccp_grid_get_{which}_device")
        self._on_stream(lambda: fn(self.h, C.byref(arr), first_row, n_rows), f"ccp_grid_get_{which}_device")
        return out

    def set_b_tensor(self, rows, first_row=None):
        """b of every channel on image rows [first_row, first_row + len(rows)) from a float32 / float64 tensor
        (rows x W x channels; first_row: the first local row, ghosts included, by default)."""
        self._set_tensor("b", rows, first_row)

    def set_x_tensor(self, rows, first_row=None):
        self._set_tensor("x", rows, first_row)

    def get_x_tensor(self, out=None, dtype=None, first_row=None, n_rows=None):
        """x of every channel as an n_rows x W x channels tensor (float64 by default; float32 rounds to nearest),
        written into `out` when given."""
        dtype = dtype or self._torch().float64
        return self._get_tensor("x", out, dtype, first_row, n_rows)

    def get_b_tensor(self, out=None, dtype=None, first_row=None, n_rows=None):
        dtype = dtype or self._torch().float64
        return self._get_tensor("b", out, dtype, first_row, n_rows)

    def assemble_rhs_tensor(self, gx, gy, constraint):
        """assemble_rhs from float32 H x W x channels tensors; constraint: one int per channel (host)."""
        torch = self._torch()
        a, _ = self._hwc(gx, "gx", (torch.float32,))
        b, _ = self._hwc(gy, "gy", (torch.float32,))
        cons = _i32(constraint)
        if cons.size != self.C:
            raise ValueError(f"constraint must hold {self.C} values")
        self._on_stream(lambda: self.L.ccp_grid_assemble_rhs_device(self.h, C.byref(a), C.byref(b), _ptr(cons)),
                        "ccp_grid_assemble_rhs_device")

    def assemble_from_images_tensor(self, images, label, init_x: bool = False):
        """assemble_from_images from a u8 N x H x W x 3 tensor (a list of H x W x 3 tensors is stacked into one,
        which costs a copy) and a u8 H x W label tensor.  Synchronises: the labels are checked on the device first."""
        torch = self._torch()
        if isinstance(images, (list, tuple)):
            images = torch.stack(list(images))
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError("images must be an N x H x W x 3 tensor")
        n = images.shape[0]
        arr, _ = self._hwc(images[0], "images", (torch.uint8,))
        arr.stride_n = images.stride(0)
        if not 1 <= n <= 256 or images.stride(0) < 0:
            raise ValueError("images must hold 1 to 256 images")
        if label.dim() == 2:
            label = label.unsqueeze(-1)
        if tuple(label.shape) != (self.H, self.W, 1):
            raise ValueError(f"label must be {self.H} x {self.W}")
        lab = self._array(label, "label", (torch.uint8,), None)
        self._on_stream(lambda: self.L.ccp_grid_assemble_from_images_device(self.h, C.byref(arr), n, C.byref(lab), 1 if init_x else 0),
                        "ccp_grid_assemble_from_images_device")

    def store_u8_tensor(self, out=None):
        """store_u8 into a u8 H x W x channels tensor (allocated when `out` is None)."""
        torch = self._torch()
        if out is None:
            with torch.cuda.device(self._device()):
                out = torch.empty((self.H, self.W, self.C), dtype=torch.uint8, device=self._device())
        arr, _ = self._hwc(out, "out", (torch.uint8,), output=True)
        self._on_stream(lambda: self.L.ccp_grid_store_u8_device(self.h, C.byref(arr)), "ccp_grid_store_u8_device")
        return out

    def set_x_u8_tensor(self, image):
        torch = self._torch()
        arr, _ = self._hwc(image, "image", (torch.uint8,))
        self._on_stream(lambda: self.L.ccp_grid_set_x_u8_device(self.h, C.byref(arr)), "ccp_grid_set_x_u8_device")

    def assemble_region_rhs_tensor(self, gx, gy, canvas, init_x: bool = False):
        """assemble_region_rhs from whole-canvas tensors: gx, gy float32, canvas u8, H x W x channels."""
        torch = self._torch()
        a, _ = self._hwc(gx, "gx", (torch.float32,))
        b, _ = self._hwc(gy, "gy", (torch.float32,))
        c, _ = self._hwc(canvas, "canvas", (torch.uint8,))
        self._on_stream(lambda: self.L.ccp_grid_assemble_region_rhs_device(self.h, C.byref(a), C.byref(b), C.byref(c), 1 if init_x else 0),
                        "ccp_grid_assemble_region_rhs_device")

    def assemble_clone_tensor(self, source, target, mixed: bool = False, init: int = 1):
        torch = self._torch()
        s_, _ = self._hwc(source, "source", (torch.uint8,))
        t_, _ = self._hwc(target, "target", (torch.uint8,))
        self._on_stream(lambda: self.L.ccp_grid_assemble_clone_device(self.h, C.byref(s_), C.byref(t_),
                                                                      CLONE_MIXED if mixed else CLONE_IMPORT, int(init)),
                        "ccp_grid_assemble_clone_device")

    def store_u8_composite_tensor(self, canvas, out=None):
        """The composite into a u8 H x W x channels tensor (allocated, zero-filled, when `out` is None); on a row block
        only the owned rows are written."""
        torch = self._torch()
        c, _ = self._hwc(canvas, "canvas", (torch.uint8,))
        if out is None:
            with torch.cuda.device(self._device()):
                out = torch.zeros((self.H, self.W, self.C), dtype=torch.uint8, device=self._device())
        o, _ = self._hwc(out, "out", (torch.uint8,), output=True)
        self._on_stream(lambda: self.L.ccp_grid_store_u8_composite_device(self.h, C.byref(c), C.byref(o)),
                        "ccp_grid_store_u8_composite_device")
        return out

    # ---- weighted grids (CCP_GRID_WEIGHTED) -----------------------------------------------------------------
    def _plane(self, a, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != (self.H, self.W):
            raise ValueError(f"{name} must be {self.H} x {self.W}")
        return a

    def set_weights(self, wx=None, wy=None, lam=None, fixed=None):
        """The operator from H x W float32 host arrays: wx weighs the edge (x,y)-(x+1,y), wy the edge (x,y)-(x,y+1), lam
        the data term; None: wx, wy 1 everywhere, lam 0.  Negative, NaN or inf weights raise CcpError (BAD_ARG) and
        leave the handle without an operator.  fixed: an H x W mask (non-zero = a pixel whose value is prescribed:
        assemble_constrained_rhs), None: no fixed pixels."""
        planes = [self._plane(a, n) for a, n in ((wx, "wx"), (wy, "wy"), (lam, "lam"))]
        stride = 4 * self.W
        if fixed is None:
            check(self.L.ccp_grid_set_weights_host(self.h, *[_ptr(p) for p in planes], stride), "ccp_grid_set_weights_host")
            return
        fixed = np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8)
        if fixed.shape != (self.H, self.W):
            raise ValueError(f"fixed must be {self.H} x {self.W}")
        check(self.L.ccp_grid_set_weights_constrained_host(self.h, *[_ptr(p) for p in planes], stride, _ptr(fixed), self.W),
              "ccp_grid_set_weights_constrained_host")

    def assemble_constrained_rhs(self, gx=None, gy=None, f=None, values=None, init_x: bool = False):
        """assemble_weighted_rhs on an operator with fixed pixels: `values` (float32 H x W x channels, None: 0) are the
        prescribed values; x := values at the fixed pixels, whose neighbours' b takes them in.  init_x: x := f on the
        live free pixels (0 on dead ones); otherwise x of the free pixels is left as it is."""
        gx = None if gx is None else self._canvas_image(gx, np.float32)
        gy = None if gy is None else self._canvas_image(gy, np.float32)
        f = None if f is None else self._canvas_image(f, np.float32)
        values = None if values is None else self._canvas_image(values, np.float32)
        row = 4 * self.W * self.C
        check(self.L.ccp_grid_assemble_constrained_rhs(self.h, _ptr(gx), _ptr(gy), row, _ptr(f), row, _ptr(values), row,
                                                       1 if init_x else 0), "ccp_grid_assemble_constrained_rhs")

    def constraint_info(self, channel=None):
        """(fixed pixels, free pixels with a non-empty row, edges with exactly one fixed end) of the installed operator;
        channel: of that channel's operator (None: channel 0, the shared operator's call)."""
        n = [C.c_int64() for _ in range(3)]
        if channel is None:
            check(self.L.ccp_grid_constraint_info(self.h, *[C.byref(v) for v in n]), "ccp_grid_constraint_info")
        else:
            check(self.L.ccp_grid_constraint_info_channel(self.h, channel, *[C.byref(v) for v in n]), "ccp_grid_constraint_info_channel")
        return tuple(v.value for v in n)

    def operator_channels(self) -> int:
        """1: one operator shared by all channels (set_weights*); channels: one per channel (set_weights_per_channel_tensor)."""
        n = C.c_int32()
        check(self.L.ccp_grid_operator_channels(self.h, C.byref(n)), "ccp_grid_operator_channels")
        return n.value

    def assemble_weighted_rhs(self, gx=None, gy=None, f=None, init_x: bool = False):
        """b of every channel from float32 H x W x channels host arrays: guidance gx, gy (None: 0) and data f (None: 0);
        init_x: x := f on live pixels (0 on dead ones)."""
        gx = None if gx is None else self._canvas_image(gx, np.float32)
        gy = None if gy is None else self._canvas_image(gy, np.float32)
        f = None if f is None else self._canvas_image(f, np.float32)
        row = 4 * self.W * self.C
        check(self.L.ccp_grid_assemble_weighted_rhs(self.h, _ptr(gx), _ptr(gy), row, _ptr(f), row, 1 if init_x else 0),
              "ccp_grid_assemble_weighted_rhs")

    def _weight_array(self, t, name, output=False):
        """ccp_device_array of an H x W float32 / float64 tensor (a broadcast view of a scalar is fine), or None."""
        torch = self._torch()
        return self._array(t, name, (torch.float32, torch.float64), (self.H, self.W), output=output)

    def _mask_array(self, fixed, name="fixed"):
        """ccp_device_array of an H x W uint8, bool, float32 or float64 mask tensor."""
        torch = self._torch()
        if isinstance(fixed, torch.Tensor) and fixed.dtype == torch.bool:
            fixed = fixed.view(torch.uint8)
        if isinstance(fixed, torch.Tensor) and fixed.dtype == torch.uint8:
            return self._array(fixed, name, (torch.uint8,), (self.H, self.W))
        return self._weight_array(fixed, name)

    def _channel_array(self, t, name, dtypes, output=False):
        """ccp_device_array of an H x W x channels tensor of the per-channel calls; an H x W tensor (an expanded scalar
        too) is passed with stride_c = 0: every channel reads the one plane.  bool is read as uint8."""
        if t is None:
            return None
        torch = self._torch()
        if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
            t = t.view(torch.uint8)
        if isinstance(t, torch.Tensor) and t.dim() == 2 and not output:
            t = t.unsqueeze(-1).expand(-1, -1, self.C)
        return self._hwc(t, name, dtypes, output=output)[0]

    def _operator_marshal(self, tensors, n_op=None):
        """How the operator-shaped arguments of a call are passed.  Returns (per_channel, arr): per_channel when the handle
        has one operator per channel (n_op, by default operator_channels(), > 1), or has one channel and any of `tensors`
        has 3 dimensions (one channel: the two layouts address the same elements and the library says 1 for both, so the
        tensors decide); arr(t, name, kind) is the ccp_device_array of a weight ("plane"), a mask of fixed pixels ("mask")
        or an output ("out"), None for None: H x W on a shared operator, H x W x channels on one per channel."""
        torch = self._torch()
        n_op = self.operator_channels() if n_op is None else n_op
        per_channel = n_op > 1 or (self.C == 1 and any(isinstance(t, torch.Tensor) and t.dim() == 3 for t in tensors))
        floats = (torch.float32, torch.float64)

        def arr(t, name, kind="plane"):
            if per_channel:
                return self._channel_array(t, name, (torch.uint8,) + floats if kind == "mask" else floats, output=kind == "out")
            if kind == "mask":
                return None if t is None else self._mask_array(t, name)
            return self._weight_array(t, name, output=kind == "out")
        return per_channel, arr

    def set_weights_per_channel_tensor(self, wx=None, wy=None, lam=None, fixed=None):
        """One operator PER CHANNEL from H x W x channels float32 / float64 tensors (an H x W tensor or an expanded scalar
        serves every channel); fixed: H x W x channels uint8, bool, float32 or float64 (!= 0: fixed), None: no fixed
        pixels.  Channel c then behaves, bit for bit, as a one-channel handle given channel c's slices through
        set_weights_tensor.  Synchronises (the verdict); a bad weight in any channel raises CcpError (BAD_ARG) and leaves
        the handle without an operator.  set_weights* returns to the shared operator."""
        torch = self._torch()
        floats = (torch.float32, torch.float64)
        arrs = [self._channel_array(t, n, floats) for t, n in ((wx, "wx"), (wy, "wy"), (lam, "lam"))]
        arrs.append(self._channel_array(fixed, "fixed", (torch.uint8,) + floats))
        self._on_stream(lambda: self.L.ccp_grid_set_weights_per_channel_device(self.h, *_refs(arrs)),
                        "ccp_grid_set_weights_per_channel_device")

    def set_mask_tensor(self, mask):
        """set_mask from an H x W uint8, bool, float32 or float64 tensor of the whole canvas (!= 0: inside the region),
        any strides, read on the device: the mask is never copied to the host.  Synchronises once (two counters)."""
        m = self._mask_array(mask, "mask")
        self._on_stream(lambda: self.L.ccp_grid_set_mask_device(self.h, C.byref(m)), "ccp_grid_set_mask_device")

    def set_weights_tensor(self, wx=None, wy=None, lam=None, fixed=None):
        """set_weights from H x W float32 / float64 tensors (expanded scalars broadcast); synchronises (the verdict).
        fixed: an H x W uint8, bool, float32 or float64 tensor (!= 0: fixed), read on the device; None: no fixed pixels."""
        refs = _refs([self._weight_array(t, n) for t, n in ((wx, "wx"), (wy, "wy"), (lam, "lam"))])
        if fixed is None:
            self._on_stream(lambda: self.L.ccp_grid_set_weights_device(self.h, *refs), "ccp_grid_set_weights_device")
            return
        m = self._mask_array(fixed)
        self._on_stream(lambda: self.L.ccp_grid_set_weights_constrained_device(self.h, *refs, C.byref(m)),
                        "ccp_grid_set_weights_constrained_device")

    def refresh_weights_tensor(self, wx=None, wy=None, lam=None):
        """New VALUES for the installed operator and everything mg_prepare derived from it, enqueued on torch's current
        stream: no allocation and no synchronisation, so torch.cuda.graph may record it.  The operator's kind (shared:
        H x W tensors; per channel: H x W x channels, an H x W tensor serves every channel), the fixed pixels, the
        hierarchy kind and every mode stay; None takes the setters' defaults.  Needs an installed operator and mg_prepare
        (CcpError STATE otherwise).  The verdict stays on the device: operator_status(), or field 5 of the enqueue solve's
        report.  A refused refresh poisons the operator until the next good one; it never drops it."""
        _, arr = self._operator_marshal((wx, wy, lam))
        refs = _refs([arr(t, n) for t, n in ((wx, "wx"), (wy, "wy"), (lam, "lam"))])
        self._on_stream(lambda: self.L.ccp_grid_refresh_weights_device(self.h, *refs), "ccp_grid_refresh_weights_device")

    def reserve_constraints(self, on=True):
        """Keep the three constraint planes of every operator the setters install from now on, fixed pixels or none, so
        that refresh_constrained_tensor can give the handle a fixed set later.  Host state only; takes effect at the
        next set_weights*; every result of the handle stays what it was, bit for bit.  24 bytes per pixel and operator."""
        check(self.L.ccp_grid_reserve_constraints(self.h, 1 if on else 0), "ccp_grid_reserve_constraints")

    def refresh_constrained_tensor(self, wx=None, wy=None, lam=None, fixed=None):
        """refresh_weights_tensor with a new set of fixed pixels: `fixed` as the setters read it (uint8, bool, float32 or
        float64, != 0: fixed; H x W, or H x W x channels on an operator per channel; None: no pixel fixed).  Enqueued on
        torch's current stream: no allocation and no synchronisation, so torch.cuda.graph may record it.  Needs what
        refresh_weights_tensor needs and the constraint planes: reserve_constraints() before the setter, or a setter's
        mask with a fixed pixel (CcpError STATE otherwise).  Afterwards the handle holds what the setter with the same
        four tensors and mg_prepare form on a fresh reserved handle, bit for bit; constraint_info reports the new set."""
        _, arr = self._operator_marshal((wx, wy, lam, fixed))
        refs = _refs([arr(t, n) for t, n in ((wx, "wx"), (wy, "wy"), (lam, "lam"))] + [arr(fixed, "fixed", "mask")])
        self._on_stream(lambda: self.L.ccp_grid_refresh_constrained_device(self.h, *refs), "ccp_grid_refresh_constrained_device")

    def reweight_tensor(self, penalty, coupling, scale, epsilon, u=None, gx=None, gy=None, base_wx=None, base_wy=None, lam=None,
                        out_wx=None, out_wy=None):
        """refresh_weights_tensor with weights formed on the device from the solution (ccp_grid_reweight_device): per edge
        w = base * (scale * phi(q)), q the squared residual gx - (uE - u) (gy, uS to the south) summed over the channels --
        all of them on a shared operator, channel c alone on an operator per channel.  penalty: "charbonnier"
        (phi = 1 / sqrt(q + epsilon^2)), "huber" (1 / max(sqrt(q), epsilon)) or "reciprocal" (1 / (sqrt(q) + epsilon));
        coupling: "edge" (each edge from its own q) or "pixel" (both forward edges of a pixel from q_x + q_y); an unknown
        name is a ValueError before any tensor is looked at.  u: None reads the handle's x, else a uint8 / float32 / float64
        H x W x channels tensor (H x W: every channel's); gx, gy: float32 H x W x channels or None (0); base_wx, base_wy,
        lam: as refresh_weights_tensor's wx, wy, lam (None: 1, 1, 0); out_wx, out_wy: float32 / float64 tensors, H x W on a
        shared operator and H x W x channels on one per channel, that receive the weights formed (not overlapping any
        input).  Enqueued on torch's current stream: no allocation, no synchronisation; the verdict is operator_status()."""
        ids = reweight_ids(penalty, coupling)
        self._reweight(ids, scale, epsilon, u, gx, gy, base_wx, base_wy, lam, out_wx, out_wy)

    def _reweight(self, ids, scale, epsilon, u, gx, gy, base_wx, base_wy, lam, out_wx, out_wy, data=None):
        """reweight_tensor (data None: ccp_grid_reweight_device) and reweight_robust_tensor (data: data_scale, data_epsilon,
        f, out_lambda; ccp_grid_reweight_robust_device) behind their checks of the names."""
        torch = self._torch()
        any_ = (torch.uint8, torch.float32, torch.float64)
        named = ((base_wx, "base_wx"), (base_wy, "base_wy"), (lam, "lam"))
        outs = ((out_wx, "out_wx"), (out_wy, "out_wy")) + (((data[3], "out_lambda"),) if data else ())
        _, arr = self._operator_marshal([t for t, _ in named + outs])
        arrs = {"u": self._channel_array(u, "u", any_), "f": self._channel_array(data[2], "f", any_) if data else None,
                "gx": self._image(gx, "gx", (torch.float32,)), "gy": self._image(gy, "gy", (torch.float32,))}
        arrs.update({n: arr(t, n) for t, n in named})
        arrs.update({n: arr(t, n, "out") for t, n in outs})
        arrs["lambda"] = arrs.pop("lam")
        ptr = lambda n: None if arrs[n] is None else C.pointer(arrs[n])
        how = Reweight(ids[0], ids[1], float(scale), float(epsilon), *[ptr(n) for n in REWEIGHT_VIEWS])
        if data is None:
            self._on_stream(lambda: self.L.ccp_grid_reweight_device(self.h, C.byref(how)), "ccp_grid_reweight_device")
            return
        rob = ReweightData(ids[2], 0, float(data[0]), 0.0 if data[1] is None else float(data[1]), ptr("f"), ptr("out_lambda"))
        self._on_stream(lambda: self.L.ccp_grid_reweight_robust_device(self.h, C.byref(how), C.byref(rob)), "ccp_grid_reweight_robust_device")

    def reweight_robust_tensor(self, penalty, coupling, scale, epsilon, data_penalty, data_scale, data_epsilon, f=None, u=None, gx=None,
                               gy=None, base_wx=None, base_wy=None, lam=None, out_wx=None, out_wy=None, out_lambda=None):
        """reweight_tensor with the data term reweighted in the same pass (ccp_grid_reweight_robust_device): the edges as
        reweight_tensor forms them, and per pixel lambda = lam * (data_scale * phi_d(dq)), dq the sum of (f - u)^2 over the
        channels (all of them on a shared operator, channel c alone on an operator per channel); lam None: 1.  penalty and
        data_penalty: "charbonnier" | "huber" | "reciprocal" | "quadratic" (phi = 1: that term is not reweighted, and its
        epsilon is not read); f: uint8 / float32 / float64 H x W x channels (H x W: every channel's), None only with
        data_penalty "quadratic"; out_lambda: a float32 / float64 tensor shaped as out_wx that receives the lambda formed,
        fixed pixels included.  The other arguments, the stream and the verdict: as reweight_tensor's."""
        ids = robust_ids(penalty, coupling, data_penalty)
        self._reweight(ids, scale, epsilon, u, gx, gy, base_wx, base_wy, lam, out_wx, out_wy, data=(data_scale, data_epsilon, f, out_lambda))

    def reweight_adjoint_tensor(self, penalty, coupling, scale, epsilon, u, gx=None, gy=None, base_wx=None, base_wy=None, lam=None,
                                data_penalty=None, data_scale=1.0, data_epsilon=None, f=None, grad_wx=None, grad_wy=None, grad_lambda=None,
                                want=("u", "gx", "gy", "base_wx", "base_wy"), out=None, dtype=None):
        """The backward pass of reweight_tensor (data_penalty None) or reweight_robust_tensor in one launch
        (ccp_grid_reweight_adjoint_device): from the upstream gradients grad_wx, grad_wy (and grad_lambda) of the weights
        formed -- float32 / float64, shaped as the weights, None: 0 -- the gradients with respect to what they were formed
        from.  The forward's arguments as the forward took them, but `u` is required (the tensor the weights were formed
        from).  want: of "u", "gx", "gy", "f" (H x W x channels) and "base_wx", "base_wy", "lam" (H x W on a shared
        operator, H x W x channels on one per channel); "f" and "lam" (the base lambda's) need data_penalty.  Only those
        are computed.  Returns {name: tensor}; a tensor given in `out` ({name: tensor}, float32 or float64, any
        non-overlapping view that shares no bytes with an input) is filled, the others are allocated as `dtype` (float64
        by default).  Enqueued on torch's current stream; the handle's operator, x and b are not touched."""
        torch = self._torch()
        ids = reweight_ids(penalty, coupling) if data_penalty is None else robust_ids(penalty, coupling, data_penalty)
        want, out = tuple(want), dict(out or {})
        planes, images = ("base_wx", "base_wy", "lam"), ("u", "gx", "gy", "f")
        unknown = [n for n in want if n not in planes + images] + [n for n in out if n not in want]
        if unknown:
            raise ValueError(f"unknown or unrequested gradients: {unknown}")
        if data_penalty is None and (grad_lambda is not None or "f" in want or "lam" in want):
            raise ValueError("grad_lambda and the gradients of f and lam need data_penalty")
        if u is None:
            raise ValueError("u is required: the tensor the weights were formed from")
        floats, any_ = (torch.float32, torch.float64), (torch.uint8, torch.float32, torch.float64)
        named = ((base_wx, "base_wx"), (base_wy, "base_wy"), (lam, "lam"), (grad_wx, "grad_wx"), (grad_wy, "grad_wy"), (grad_lambda, "grad_lambda"))
        per_channel, arr = self._operator_marshal([t for t, _ in named] + [out.get(n) for n in planes])
        arrs = {"u": self._channel_array(u, "u", any_), "f": self._channel_array(f, "f", any_),
                "gx": self._image(gx, "gx", (torch.float32,)), "gy": self._image(gy, "gy", (torch.float32,)), "out_wx": None, "out_wy": None}
        arrs.update({n: arr(t, n) for t, n in named})
        arrs["lambda"] = arrs.pop("lam")
        result, outs = {}, {}
        for n in want:
            t = out.get(n)
            if t is None:
                shape = (self.H, self.W) if n in planes and not per_channel else (self.H, self.W, self.C)
                with torch.cuda.device(self._device()):
                    t = torch.empty(shape, dtype=dtype or torch.float64, device=self._device())
            plane = n in planes and not per_channel
            outs["g_lambda" if n == "lam" else "g_" + n] = arr(t, n, "out") if plane else self._hwc(t, n, floats, output=True)[0]
            result[n] = t
        ptr = lambda d, n: None if d.get(n) is None else C.pointer(d[n])
        how = Reweight(ids[0], ids[1], float(scale), float(epsilon), *[ptr(arrs, n) for n in REWEIGHT_VIEWS])
        io = ReweightGrads(*([ptr(arrs, n) for n in REWEIGHT_GRADS_IN] + [ptr(outs, n) for n in REWEIGHT_GRADS_OUT]))
        rob = None
        if data_penalty is not None:
            rob = ReweightData(ids[2], 0, float(data_scale), 0.0 if data_epsilon is None else float(data_epsilon), ptr(arrs, "f"), None)
        self._on_stream(lambda: self.L.ccp_grid_reweight_adjoint_device(self.h, C.byref(how), None if rob is None else C.byref(rob), C.byref(io)),
                        "ccp_grid_reweight_adjoint_device")
        return result

    def irls_adjoint_step_tensor(self, penalty, coupling, scale, epsilon, u, grad, gx=None, gy=None, base_wx=None, base_wy=None, lam=None,
                                 data_penalty=None, data_scale=1.0, data_epsilon=None, f=None, fixed=None, report=None):
        """One step z := G + J'z of the adjoint iteration at an IRLS fixed point, in one launch
        (ccp_grid_irls_adjoint_step_device): with v in the handle's x (the solution of A v = z_old) and z_old in its b, b
        becomes G + g_u on the free live pixels and 0 elsewhere, g_u what weighted_adjoint_tensor's "wx", "wy" ("lam")
        gradients of (v, u) and then reweight_adjoint_tensor's "u" gradient of those give, bit for bit; x is left alone,
        so the next enqueue solve starts from the previous v.  The reweight's arguments as reweight_adjoint_tensor takes
        them (`u`: the fixed point, required); grad: G = dL/du, float32 / float64 H x W x channels; fixed: the mask as
        weighted_adjoint_tensor takes it; report: None or a float64 channels x 2 tensor that receives
        (sum (z_new - z_old)^2, sum z_new^2) per channel over its free live pixels, the same bits for the same inputs.
        Needs mg_prepare (CcpError STATE otherwise).  Enqueued on torch's current stream: no allocation, no
        synchronisation."""
        torch = self._torch()
        ids = reweight_ids(penalty, coupling) if data_penalty is None else robust_ids(penalty, coupling, data_penalty)
        if u is None or grad is None:
            raise ValueError("u (the fixed point) and grad (dL/du) are required")
        floats, any_ = (torch.float32, torch.float64), (torch.uint8, torch.float32, torch.float64)
        named = ((base_wx, "base_wx"), (base_wy, "base_wy"), (lam, "lam"))
        _, arr = self._operator_marshal([t for t, _ in named] + [fixed])
        arrs = {"u": self._channel_array(u, "u", any_), "f": self._channel_array(f, "f", any_),
                "gx": self._image(gx, "gx", (torch.float32,)), "gy": self._image(gy, "gy", (torch.float32,)), "out_wx": None, "out_wy": None}
        arrs.update({n: arr(t, n) for t, n in named})
        arrs["lambda"] = arrs.pop("lam")
        ptr = lambda a: None if a is None else C.pointer(a)
        how = Reweight(ids[0], ids[1], float(scale), float(epsilon), *[ptr(arrs[n]) for n in REWEIGHT_VIEWS])
        rob = None
        if data_penalty is not None:
            rob = ReweightData(ids[2], 0, float(data_scale), 0.0 if data_epsilon is None else float(data_epsilon), ptr(arrs["f"]), None)
        rep = self._enqueue_report(report, 2)
        step =IrlsAdjointStep(ptr(self._hwc(grad, "grad", floats)[0]), ptr(arr(fixed, "fixed", "mask")), ptr(rep))
        self._on_stream(lambda: self.L.ccp_grid_irls_adjoint_step_device(self.h, C.byref(how), None if rob is None else C.byref(rob),
                                                                         C.byref(step)), "ccp_grid_irls_adjoint_step_device")

    def operator_status(self) -> int:
        """The operator status word of the last refresh_weights_tensor (0: good; 1: a bad weight, 2: out of float range in
        "f32" precision, 4: not floating in "constant" null-space mode, summed); 0 after a setter.  Synchronises."""
        word = C.c_int32()
        self._on_stream(lambda: self.L.ccp_grid_operator_status(self.h, C.byref(word)), "ccp_grid_operator_status")
        return word.value

    def assemble_constrained_rhs_tensor(self, gx=None, gy=None, f=None, values=None, init_x: bool = False):
        """assemble_constrained_rhs from H x W x channels tensors: gx, gy float32; f and values u8, float32 or float64."""
        torch = self._torch()
        any_ = (torch.uint8, torch.float32, torch.float64)
        refs = _refs([self._image(gx, "gx", (torch.float32,)), self._image(gy, "gy", (torch.float32,)), self._image(f, "f", any_),
                      self._image(values, "values", any_)])
        self._on_stream(lambda: self.L.ccp_grid_assemble_constrained_rhs_device(self.h, *refs, 1 if init_x else 0),
                        "ccp_grid_assemble_constrained_rhs_device")

    def assemble_weighted_rhs_tensor(self, gx=None, gy=None, f=None, init_x: bool = False):
        """assemble_weighted_rhs from H x W x channels tensors: gx, gy float32, f u8, float32 or float64."""
        torch = self._torch()
        refs = _refs([self._image(gx, "gx", (torch.float32,)), self._image(gy, "gy", (torch.float32,)),
                      self._image(f, "f", (torch.uint8, torch.float32, torch.float64))])
        self._on_stream(lambda: self.L.ccp_grid_assemble_weighted_rhs_device(self.h, *refs, 1 if init_x else 0),
                        "ccp_grid_assemble_weighted_rhs_device")

    # ---- the backward pass of a weighted solve (ccp_gs.h, "Differentiating a weighted solve") ---------------------
    def adjoint_begin_tensor(self, grad):
        """Load the adjoint right-hand side: b := grad (float32 / float64 H x W x channels, dL/du) on free live pixels and
        0 on fixed and dead ones, x := 0.  mg_conjugate_gradient then leaves the adjoint solution v in x."""
        torch = self._torch()
        arr, _ = self._hwc(grad, "grad", (torch.float32, torch.float64))
        self._on_stream(lambda: self.L.ccp_grid_adjoint_begin_device(self.h, C.byref(arr)), "ccp_grid_adjoint_begin_device")

    def weighted_adjoint_tensor(self, u, grad=None, gx=None, gy=None, f=None, wx=None, wy=None, lam=None, fixed=None,
                                want=("wx", "wy", "lam", "gx", "gy", "f", "values"), out=None, dtype=None):
        """The gradients of a weighted solve in one pass, from the forward composite `u` (float64 H x W x channels), the
        adjoint solution in the handle's x, and the inputs of the forward solve as they were installed (gx, gy, f as
        assemble_constrained_rhs_tensor takes them; wx, wy, lam, fixed as set_weights_tensor takes them).  want: which
        gradients to compute, of "wx", "wy", "lam" (H x W) and "gx", "gy", "f", "values" (H x W x channels); "values"
        needs `grad` (dL/du).  Only those are computed, and only the inputs they need are read.  Returns {name: tensor};
        a tensor given in `out` ({name: tensor}, float32 or float64, any non-overlapping view) is filled, the others are
        allocated as `dtype` (float64 by default).  On a handle with one operator per channel
        (set_weights_per_channel_tensor) wx, wy, lam, fixed are H x W x channels (H x W: every channel's) and the
        gradients "wx", "wy", "lam" come back H x W x channels, channel c's from channel c alone."""
        torch = self._torch()
        want = tuple(want)
        n_op = C.c_int32(1)                                          # (no operator, not weighted: the call below refuses)
        if self.L.ccp_grid_operator_channels(self.h, C.byref(n_op)) != 0:
            n_op.value = 1
        per_channel, arr = self._operator_marshal([wx, wy, lam, fixed] + [(out or {}).get(n) for n in ("wx", "wy", "lam")], n_op.value)
        planes, images = ("wx", "wy", "lam"), ("gx", "gy", "f", "values")
        unknown = [n for n in want if n not in planes + images] + [n for n in (out or {}) if n not in want]
        if unknown:
            raise ValueError(f"unknown or unrequested gradients: {unknown}")
        if "values" in want and grad is None:
            raise ValueError("the gradient of values needs grad")
        floats, any_ = (torch.float32, torch.float64), (torch.uint8, torch.float32, torch.float64)
        ins = {"u": self._hwc(u, "u", (torch.float64,))[0], "grad_x": self._image(grad, "grad", floats),
               "gx": self._image(gx, "gx", (torch.float32,)), "gy": self._image(gy, "gy", (torch.float32,)), "f": self._image(f, "f", any_),
               "wx": arr(wx, "wx"), "wy": arr(wy, "wy"), "lambda": arr(lam, "lam"), "fixed": arr(fixed, "fixed", "mask")}
        result, outs = {}, {}
        for n in want:
            t = (out or {}).get(n)
            if t is None:
                shape = (self.H, self.W) if n in planes and not per_channel else (self.H, self.W, self.C)
                with torch.cuda.device(self._device()):
                    t = torch.empty(shape, dtype=dtype or torch.float64, device=self._device())
            plane = n in planes and not per_channel
            outs["g_lambda" if n == "lam" else "g_" + n] = arr(t, n, "out") if plane else self._hwc(t, n, floats, output=True)[0]
            result[n] = t
        a = AdjointInputs(*[None if ins[n] is None else C.pointer(ins[n]) for n in ADJOINT_INPUTS])
        b = AdjointOutputs(*[None if outs.get(n) is None else C.pointer(outs[n]) for n in ADJOINT_OUTPUTS])
        self._on_stream(lambda: self.L.ccp_grid_weighted_adjoint_device(self.h, C.byref(a), C.byref(b)),
                        "ccp_grid_weighted_adjoint_device")
        return result

    def region_begin(self):
        check(self.L.ccp_grid_region_begin(self.h), "ccp_grid_region_begin")

    def region_end(self):
        """(device ms, sweep launches, iterations of the fused passes) since region_begin — HIP events on
        the handle's stream."""
        ms, n, it = C.c_float(), C.c_int64(), C.c_int64()
        check(self.L.ccp_grid_region_end(self.h, C.byref(ms), C.byref(n), C.byref(it)), "ccp_grid_region_end")
        return ms.value, n.value, it.value

    # ---- row blocks over RCCL (ccp_comm_*) ------------------------------------------------------
    def attach_comm(self, comm: "Comm"):
        check(self.L.ccp_grid_attach_comm(self.h, comm.h if comm is not None else None), "ccp_grid_attach_comm")
        self._comm = comm                       # the communicator must outlive the attachment

    def set_overlap(self, on: bool):
        check(self.L.ccp_grid_set_overlap(self.h, 1 if on else 0), "ccp_grid_set_overlap")

    def exchange_halos(self):
        check(self.L.ccp_grid_exchange_halos(self.h), "ccp_grid_exchange_halos")

    def sweep_rowblocked(self, iterations: int):
        check(self.L.ccp_grid_sweep_rowblocked(self.h, iterations), "ccp_grid_sweep_rowblocked")

    def gauss_seidel_rowblocked(self, epsilon=1e-6, max_iteration=1000, check_every=1):
        reps = (Report * self.C)()
        check(self.L.ccp_grid_gauss_seidel_rowblocked(self.h, epsilon, max_iteration, check_every, reps),
              "ccp_grid_gauss_seidel_rowblocked")
        return list(reps)

    def conjugate_gradient_rowblocked(self, epsilon=1e-16, max_iteration=1000):
        reps = (Report * self.C)()
        check(self.L.ccp_grid_conjugate_gradient_rowblocked(self.h, epsilon, max_iteration, reps), "ccp_grid_conjugate_gradient_rowblocked")
        return list(reps)

    def mg_conjugate_gradient_rowblocked(self, epsilon, max_iteration, smoothing_sweeps=2):
        """Multigrid-preconditioned CG on the partitioned system (collective; one Report per channel)."""
        reps = (Report * self.C)()
        check(self.L.ccp_grid_mg_conjugate_gradient_rowblocked(self.h, epsilon, max_iteration, smoothing_sweeps, reps),
              "ccp_grid_mg_conjugate_gradient_rowblocked")
        return list(reps)

    def mg_apply_rowblocked(self, smoothing_sweeps=2):
        """x := M^-1 b on the owned rows (one V-cycle per channel across the blocks; collective, diagnostic)."""
        check(self.L.ccp_grid_mg_apply_rowblocked(self.h, smoothing_sweeps), "ccp_grid_mg_apply_rowblocked")

    def mg_rowblock_info(self):
        """(levels, distributed levels, (width, height) of the first level every rank holds whole) — collective."""
        n, d, w, h = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.ccp_grid_mg_rowblock_info(self.h, C.byref(n), C.byref(d), C.byref(w), C.byref(h)), "ccp_grid_mg_rowblock_info")
        return n.value, d.value, (w.value, h.value)

    def residual_norm2_global(self):
        out = np.empty(2 * self.C, dtype=np.float64)
        check(self.L.ccp_grid_residual_norm2_global(self.h, _ptr(out)), "ccp_grid_residual_norm2_global")
        return out[:self.C].copy(), out[self.C:].copy()

    def comm_stats(self):
        """(exchanges issued, wait mode: 0 hipStreamWaitValue64 / 1 polling kernel / -1 none, rows sent up, down)."""
        n, mode, up, down = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.ccp_grid_comm_stats(self.h, C.byref(n), C.byref(mode), C.byref(up), C.byref(down)), "ccp_grid_comm_stats")
        return n.value, mode.value, up.value, down.value

    def last_timing(self):
        ms, n = C.c_float(), C.c_int32()
        check(self.L.ccp_grid_last_timing(self.h, C.byref(ms), C.byref(n)), "ccp_grid_last_timing")
        return ms.value, n.value


# ---- lab8's panorama merge on torch tensors (ccp_panorama_*_device, ccp_mask_erode_cross_device) -----------------------
# Free functions: every tensor lives on one GPU, any non-negative strides (interleaved, planar-permuted, a window of a
# larger tensor); each call is enqueued on torch.cuda.current_stream() of that GPU with no host synchronisation.
def _pano_array(t, name, dtype, shape, dev, output=False):
    """Check tensor `t` (H x W x C, or H x W when shape[2] == 1) and return its ccp_device_array."""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a torch tensor on a GPU")
    if t.device.index != dev:
        raise ValueError(f"{name} must be on cuda:{dev}, not {t.device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must have dtype {dtype}, not {t.dtype}")
    if t.dim() == 2 and shape[2] == 1:
        t = t.unsqueeze(-1)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {' x '.join(str(n) for n in shape)}, not {tuple(t.shape)}")
    if any(s < 0 for s in t.stride()):
        raise ValueError(f"{name} has a negative stride")
    if output and not _no_overlap(t.shape, t.stride()):
        raise ValueError(f"{name} is an output whose elements overlap")
    sy, sx, sc = t.stride()
    return DeviceArray(t.data_ptr(), DTYPE_F32 if dtype == torch.float32 else DTYPE_U8, 0, 0, sy, sx, sc)


def _pano_stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream)


def _pano_state(state):
    """(PanoramaState, device, H, W, C, the ccp_device_arrays kept alive) of a (dx, dy, raw, mask) tuple."""
    import torch
    dx, dy, raw, mask = state
    if not isinstance(raw, torch.Tensor) or raw.device.type != "cuda" or raw.dim() not in (2, 3):
        raise ValueError("raw must be an H x W x C torch tensor on a GPU")
    dev = raw.device.index
    H, W = raw.shape[0], raw.shape[1]
    ch = raw.shape[2] if raw.dim() == 3 else 1
    if ch not in (1, 3):
        raise ValueError("the merge serves 1 or 3 channels")
    arrs = [_pano_array(dx, "dx", torch.float32, (H, W, ch), dev, True), _pano_array(dy, "dy", torch.float32, (H, W, ch), dev, True),
            _pano_array(raw, "raw", torch.uint8, (H, W, ch), dev, True), _pano_array(mask, "mask", torch.uint8, (H, W, 1), dev, True)]
    return PanoramaState(W, H, ch, 0, *[C.pointer(a) for a in arrs]), dev, H, W, ch, arrs


def mask_erode_cross_tensor(mask, times: int, out=None):
    """`times` (1..8) cross erosions of a u8 H x W mask tensor in one launch (lab8_workload.erode_cross, repeated):
    255 where every canvas pixel within L1 distance `times` is set, else 0."""
    import torch
    if not isinstance(mask, torch.Tensor) or mask.device.type != "cuda" or mask.dim() != 2:
        raise ValueError("mask must be an H x W torch tensor on a GPU")
    if not 1 <= int(times) <= 8:
        raise ValueError("times must be 1..8")
    dev = mask.device.index
    H, W = mask.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=mask.device)
    a = _pano_array(mask, "mask", torch.uint8, (H, W, 1), dev)
    b = _pano_array(out, "out", torch.uint8, (H, W, 1), dev, True)
    check(load().ccp_mask_erode_cross_device(dev, _pano_stream(dev), W, H, C.byref(a), C.byref(b), int(times)),
          "ccp_mask_erode_cross_device")
    return out


def panorama_begin_tensor(img0, mask0, out=None):
    """The merge state (dx, dy, raw, mask) of the first image: u8 H x W x C colours and its u8 H x W footprint mask.
    out: four tensors to write into (float32, float32, u8 H x W x C and u8 H x W), allocated when None."""
    import torch
    if not isinstance(img0, torch.Tensor) or img0.device.type != "cuda" or img0.dim() not in (2, 3):
        raise ValueError("img0 must be an H x W x C torch tensor on a GPU")
    if out is None:
        shape = tuple(img0.shape)
        out = (torch.empty(shape, dtype=torch.float32, device=img0.device), torch.empty(shape, dtype=torch.float32, device=img0.device),
               torch.empty(shape, dtype=torch.uint8, device=img0.device), torch.empty(shape[:2], dtype=torch.uint8, device=img0.device))
    st, dev, H, W, ch, _keep = _pano_state(out)
    a = _pano_array(img0, "img0", torch.uint8, (H, W, ch), dev)
    b = _pano_array(mask0, "mask0", torch.uint8, (H, W, 1), dev)
    check(load().ccp_panorama_begin_device(dev, _pano_stream(dev), C.byref(st), C.byref(a), C.byref(b)), "ccp_panorama_begin_device")
    return tuple(out)


def panorama_add_tensor(state, img, outer, inner):
    """One more image merged into `state` (dx, dy, raw, mask) in place, as the body of lab8_workload.merge does with
    outer = erode_mask2 and inner = erode_mask (u8 H x W)."""
    import torch
    st, dev, H, W, ch, _keep = _pano_state(state)
    a = _pano_array(img, "img", torch.uint8, (H, W, ch), dev)
    b = _pano_array(outer, "outer", torch.uint8, (H, W, 1), dev)
    c = _pano_array(inner, "inner", torch.uint8, (H, W, 1), dev)
    check(load().ccp_panorama_add_device(dev, _pano_stream(dev), C.byref(st), C.byref(a), C.byref(b), C.byref(c)),
          "ccp_panorama_add_device")


def panorama_finish_tensor(state):
    """EnforceGradientBound on `state` in place: dx, dy along the rim of the union mask recomputed from raw."""
    st, dev, _H, _W, _ch, _keep = _pano_state(state)
    check(load().ccp_panorama_finish_device(dev, _pano_stream(dev), C.byref(st)), "ccp_panorama_finish_device")
