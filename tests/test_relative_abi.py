"""CPU: the enqueue-only multigrid PCG with a stop test relative to |b| (include/ccp_gs.h,
ccp_grid_mg_conjugate_gradient_enqueue_relative) at the boundary: the header declares the function and its define and the
library exports it, the ABI version stays 6, a NULL handle is a bad argument, the header still compiles as C11 and C++17
with a use of the call, capi.Grid has the method and tensor_ops.WeightedSolver has set_stop with the stated signatures,
and the header states the contract a caller relies on.  No device is touched."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAME = "ccp_grid_mg_conjugate_gradient_enqueue_relative"


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_function():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+" + NAME + r"\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*double\s+epsilon_abs\s*,\s*double\s+epsilon_rel\s*,"
                     r"\s*int32_t\s+max_iteration\s*,\s*int32_t\s+smoothing_sweeps\s*,\s*const\s+ccp_device_array\s*\*\s*report\s*\)\s*;", text)
    assert re.search(r"#define\s+CCP_MG_RELATIVE_REPORT_FIELDS\s+8\b", text)
    # declared after the absolute call, whose declaration is still there
    assert text.index("ccp_grid_mg_conjugate_gradient_enqueue(") < text.index(NAME + "(")
    lib = capi.load()
    assert hasattr(lib, NAME)
    assert NAME in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive


def test_null_handle_is_a_bad_argument():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    for cap in (0, 10, 4097, -1):
        assert getattr(lib, NAME)(None, 0.0, 1e-8, cap, 0, None) == BAD_ARG
    assert getattr(lib, NAME)(None, -1.0, float("nan"), 10, 0, None) == BAD_ARG


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    ccp_device_array report = {0, CCP_DTYPE_F64, 0, 0, CCP_MG_RELATIVE_REPORT_FIELDS, 1, 0};\n"
            "    int a = ccp_grid_mg_prepare(0, 0);\n"
            "    int b = ccp_grid_mg_conjugate_gradient_enqueue_relative(0, 0.0, 1e-8, CCP_MG_ENQUEUE_MAX_ITERATION, 0, &report);\n"
            "    int c = ccp_grid_mg_conjugate_gradient_enqueue_relative(0, 1e-12, 1e-8, 12, 2, 0);\n"
            "    return a + b + c;\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_relative.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_method_and_set_stop_signatures():
    from coursecomputationalphotography_amd import capi, tensor_ops
    p = inspect.signature(capi.Grid.mg_conjugate_gradient_enqueue_relative).parameters
    assert list(p) == ["self", "epsilon_abs", "epsilon_rel", "max_iteration", "sweeps", "report"]
    assert p["sweeps"].default == 0 and p["report"].default is None
    p = inspect.signature(tensor_ops.WeightedSolver.set_stop).parameters
    assert list(p) == ["self", "epsilon", "relative"]
    assert p["epsilon"].default is None and p["relative"].default is None
    assert "relative" in (tensor_ops.WeightedSolver.__doc__ or "")


def test_set_stop_is_host_state_only():
    """No handle, no device: the method only records what the next solves pass on"""
    from coursecomputationalphotography_amd import tensor_ops
    s = object.__new__(tensor_ops.WeightedSolver)
    s.epsilon, s.relative = 1e-6, None
    s.set_stop(0.0, 1e-10)
    assert (s.epsilon, s.relative) == (0.0, 1e-10)
    s.set_stop(relative=1e-8)
    assert (s.epsilon, s.relative) == (0.0, 1e-8)
    s.set_stop(epsilon=1e-3)                                     # relative=None is the default: back to the absolute test
    assert (s.epsilon, s.relative) == (1e-3, None)


def test_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*(?!/)", "\n", header()).split())          # (the comment's line prefix is not text)
    start = text.index("ccp_grid_mg_conjugate_gradient_enqueue_relative: the enqueue solve above")
    doc = text[start:text.index("int " + NAME + "(")]
    for word in ("eps_c = fmax(epsilon_abs, epsilon_rel * bnorm_c)", "bnorm_c = sqrt(bb_c)", "one multiply, then fmax",
                 "r1norm < eps_c || r1norm == 0.0", "no extra pass", "BIT FOR BIT", "`channels` x 8", "[6] bnorm_c", "[7] eps_c",
                 "epsilon_rel == 0", "bit for bit", "negative, NaN or infinite", "CCP_ERR_BAD_ARG",
                 "a zero right-hand side with epsilon_abs == 0 and a non-zero x", "runs to the cap", "give epsilon_abs a floor",
                 "[6] = [7] = +0.0", "No allocation", "no host synchronisation", "ccp_grid_mg_prepare, always",
                 "Out of scope", "a synchronous relative twin", "_rowblocked", "ccp_grid_mg_apply", "the C++ facades",
                 "relative to the initial residual rather than b", "the ABI version does not change"):
        assert word in doc, word
    # the absolute call's block points here, in a parenthesis at its end
    old = text[text.index("The multigrid PCG without the host"):text.index("int ccp_grid_mg_conjugate_gradient_enqueue(")]
    assert old.rstrip().endswith("ccp_grid_mg_conjugate_gradient_enqueue_relative below.) */ #define CCP_MG_ENQUEUE_MAX_ITERATION 4096")
