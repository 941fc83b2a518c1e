"""CPU: ccp_grid_irls_adjoint_step_device (include/ccp_gs.h) at the boundary: the header declares the function and its
struct and the library exports it, the ABI version stays 6, a NULL handle is a bad argument whatever else is passed, the
header still compiles as C11 and C++17, capi.Grid, tensor_ops.WeightedSolver and tensor_ops carry the new names with their
signatures and the docstrings say what the gradient is, and the header states the contract a caller relies on.  No device
is touched."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAME = "ccp_grid_irls_adjoint_step_device"


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_function():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+ccp_grid_irls_adjoint_step_device\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*const\s+ccp_reweight\s*\*\s*how\s*,\s*"
                     r"const\s+ccp_reweight_data\s*\*\s*data\s*,\s*const\s+ccp_irls_adjoint_step\s*\*\s*step\s*\)\s*;", text)
    struct = re.search(r"typedef\s+struct\s+ccp_irls_adjoint_step\s*\{(.*?)\}\s*ccp_irls_adjoint_step\s*;", text, re.S)
    assert struct
    fields = re.findall(r"const\s+ccp_device_array\s*\*\s*(\w+)\s*;", struct.group(1))
    assert fields == ["grad_x", "fixed", "report"]
    assert [n for n, _ in capi.IrlsAdjointStep._fields_] == fields
    import ctypes as C
    assert C.sizeof(capi.IrlsAdjointStep) == 3 * C.sizeof(C.c_void_p)
    assert text.index("ccp_grid_reweight_adjoint_device(") < text.index("typedef struct ccp_irls_adjoint_step")
    lib = capi.load()
    assert hasattr(lib, NAME) and NAME in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive


def test_null_handle_is_a_bad_argument():
    import ctypes as C
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    how, data, step = capi.Reweight(), capi.ReweightData(), capi.IrlsAdjointStep()
    assert lib.ccp_grid_irls_adjoint_step_device(None, None, None, None) == BAD_ARG
    assert lib.ccp_grid_irls_adjoint_step_device(None, C.byref(how), None, C.byref(step)) == BAD_ARG
    assert lib.ccp_grid_irls_adjoint_step_device(None, C.byref(how), C.byref(data), C.byref(step)) == BAD_ARG


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    ccp_device_array w = {0, CCP_DTYPE_F64, 0, 0, 64, 1, 0};\n"
            "    ccp_reweight how = {CCP_REWEIGHT_HUBER, CCP_REWEIGHT_PIXEL, 1.0, 1e-2, &w, 0, 0, 0, 0, 0, 0, 0};\n"
            "    ccp_reweight_data data = {CCP_REWEIGHT_QUADRATIC, 0, 1.0, 0.0, 0, 0};\n"
            "    ccp_irls_adjoint_step step = {&w, 0, &w};\n"
            "    return ccp_grid_irls_adjoint_step_device(0, &how, &data, &step) + ccp_grid_irls_adjoint_step_device(0, &how, 0, &step);\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_irls_adjoint_step.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_weighted_solver_and_tensor_ops_carry_the_names():
    from coursecomputationalphotography_amd import capi, tensor_ops
    p = inspect.signature(capi.Grid.irls_adjoint_step_tensor).parameters
    assert list(p)[:7] == ["self", "penalty", "coupling", "scale", "epsilon", "u", "grad"]
    assert p["u"].default is inspect.Parameter.empty and p["grad"].default is inspect.Parameter.empty
    for name in ("gx", "gy", "base_wx", "base_wy", "lam", "data_penalty", "data_epsilon", "f", "fixed", "report"):
        assert p[name].default is None, name
    p = inspect.signature(tensor_ops.WeightedSolver.fixed_point_grad).parameters
    assert list(p)[:13] == ["self", "u", "penalty", "coupling", "scale", "epsilon", "gx", "gy", "f", "values", "base_wx", "base_wy", "data_weight"]
    for name in ("backward_steps", "backward_tolerance", "check_every", "backward_history", "strict"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["backward_steps"].default is inspect.Parameter.empty and p["backward_tolerance"].default is None
    assert p["check_every"].default == 8 and p["backward_history"].default is None and p["strict"].default is True
    unrolled = inspect.signature(tensor_ops.irls_solve_grad).parameters
    implicit = inspect.signature(tensor_ops.irls_solve_implicit).parameters
    extra = ["backward_steps", "backward_tolerance", "check_every", "backward_history"]
    assert list(implicit) == [n for n in unrolled if n != "adjoint_history"] + extra
    for fn, base in ((tensor_ops.tv_denoise_implicit, tensor_ops.tv_denoise_grad), (tensor_ops.tv_l1_denoise_implicit, tensor_ops.tv_l1_denoise_grad)):
        assert list(inspect.signature(fn).parameters) == [n for n in inspect.signature(base).parameters if n != "adjoint_history"] + extra
    for fn in (tensor_ops.irls_solve_implicit, tensor_ops.tv_denoise_implicit, tensor_ops.tv_l1_denoise_implicit,
               tensor_ops.WeightedSolver.fixed_point_grad):
        doc = " ".join(fn.__doc__.split())
        assert "fixed point" in doc and "O(||u_K - u_{K-1}||)" in doc and "truncated Neumann series" in doc, fn.__name__
    doc = " ".join(tensor_ops.irls_solve_implicit.__doc__.split())
    for word in ("the last forward step's update is read once", "at the forward's own linear rate", "no convexity guarantee"):
        assert word in doc, word


def test_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*(?!/)", "\n", header()).split())          # (the comment's line prefix is not text)
    start = text.index("Differentiating IRLS at its fixed point: one fused step of the adjoint iteration")
    assert start > text.index("int ccp_grid_reweight_adjoint_device(")       # the new section follows that declaration
    doc = text[start:text.index("typedef struct ccp_irls_adjoint_step")]
    for word in ("z_{k+1} = G + J' z_k", "how->u = u^ is required", "read as +0.0 at a fixed pixel whatever it holds there",
                 "z_old: the handle's b", "no multiply-add fused", "s = vE - v; r = gx - (uE - u); acc += s * r",
                 "a per-channel operator takes channel c alone", "accl += v * (f - u)", "+0.0 at a fixed pixel",
                 "exactly ccp_grid_reweight_adjoint_device's g_u", "the data term last", "z_new = G + g_u", "one addition",
                 "b := z_new on free live pixels and +0.0 on fixed and dead ones", "the installed d != 0",
                 "x, the operator, the hierarchy, the counts and the status word are not touched", "bit for bit", "but x is kept",
                 "report[c] = (sum (z_new - z_old)^2, sum z_new^2)", "two-stage reduction in a fixed order", "without floating-point atomics",
                 "the same inputs give the same bits", "the caller passes no workspace", "no allocation", "no memset",
                 "no host synchronisation", "no copy", "stream capture", "returns CCP_OK", "nothing enqueued and b untouched",
                 "step or step->grad_x NULL: CCP_ERR_BAD_ARG", "CCP_ERR_STATE", "CCP_ERR_UNSUPPORTED", "Out of scope",
                 "Krylov or Anderson acceleration", "Hessian-weight shortcut", "gradients with respect to the epsilons",
                 "the ABI version does not change"):
        assert word in doc, word
    assert "implicit differentiation at the IRLS fixed point" not in text     # no longer listed as not done
