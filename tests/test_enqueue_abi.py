"""CPU: the host-free multigrid PCG (include/ccp_gs.h, ccp_grid_mg_prepare / ccp_grid_mg_conjugate_gradient_enqueue) at
the boundary: the header declares both functions and the library exports them, the header still compiles as C11 and
C++17, the ABI version stays 6, a NULL handle is a bad argument, capi.Grid has the two methods, tensor_ops has the
persistent WeightedSolver with its signature, and the header states the contract a caller relies on.  No device is
touched."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAMES = ("ccp_grid_mg_prepare", "ccp_grid_mg_conjugate_gradient_enqueue")


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_functions():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+ccp_grid_mg_prepare\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s+smoothing_sweeps\s*\)\s*;", text)
    assert re.search(r"int\s+ccp_grid_mg_conjugate_gradient_enqueue\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*double\s+epsilon\s*,\s*int32_t\s+max_iteration\s*,"
                     r"\s*int32_t\s+smoothing_sweeps\s*,\s*const\s+ccp_device_array\s*\*\s*report\s*\)\s*;", text)
    assert re.search(r"#define\s+CCP_MG_ENQUEUE_MAX_ITERATION\s+4096\b", text)
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive


def test_null_handle_is_a_bad_argument():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    for sweeps in (0, 2, 9):
        assert lib.ccp_grid_mg_prepare(None, sweeps) == BAD_ARG
    for cap in (0, 10, 4097, -1):
        assert lib.ccp_grid_mg_conjugate_gradient_enqueue(None, 1e-10, cap, 0, None) == BAD_ARG


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    ccp_device_array report = {0, CCP_DTYPE_F64, 0, 0, 6, 1, 0};\n"
            "    int a = ccp_grid_mg_prepare(0, 0);\n"
            "    int b = ccp_grid_mg_conjugate_gradient_enqueue(0, 1e-10, CCP_MG_ENQUEUE_MAX_ITERATION, 0, &report);\n"
            "    int c = ccp_grid_mg_conjugate_gradient_enqueue(0, 1e-10, 12, 2, 0);\n"
            "    return a + b + c;\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_enqueue.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_has_the_two_methods():
    from coursecomputationalphotography_amd import capi
    p = inspect.signature(capi.Grid.mg_prepare).parameters
    assert list(p) == ["self", "sweeps"] and p["sweeps"].default == 0
    p = inspect.signature(capi.Grid.mg_conjugate_gradient_enqueue).parameters
    assert list(p) == ["self", "epsilon", "max_iteration", "sweeps", "report"]
    assert p["sweeps"].default == 0 and p["report"].default is None


def test_tensor_ops_has_the_persistent_solver():
    from coursecomputationalphotography_amd import tensor_ops
    p = inspect.signature(tensor_ops.WeightedSolver.__init__).parameters
    assert list(p) == ["self", "H", "W", "C", "device", "iterations", "epsilon", "hierarchy", "precision", "channels", "smoother", "nullspace"]
    for name in ("iterations", "epsilon", "hierarchy", "precision", "channels", "smoother", "nullspace"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["iterations"].default is inspect.Parameter.empty and p["epsilon"].default is inspect.Parameter.empty
    assert [p[n].default for n in ("hierarchy", "precision", "channels", "smoother", "nullspace")] == ["rescaled", "f64", "sequential", "point", "none"]
    p = inspect.signature(tensor_ops.WeightedSolver.set_operator).parameters
    assert list(p) == ["self", "wx", "wy", "data_weight", "fixed"] and p["data_weight"].default is None and p["fixed"].default is None
    p = inspect.signature(tensor_ops.WeightedSolver.solve).parameters
    assert list(p) == ["self", "gx", "gy", "f", "values", "x0", "out", "report"]
    assert all(p[n].default is None for n in ("values", "x0", "out", "report"))
    p = inspect.signature(tensor_ops.WeightedSolver.solve_grad).parameters
    assert list(p)[:6] == ["self", "gx", "gy", "f", "values", "x0"] and "report" in p and "strict" not in p
    for name in ("close", "__enter__", "__exit__"):
        assert hasattr(tensor_ops.WeightedSolver, name), name


def test_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*(?!/)", "\n", header()).split())          # (the comment's line prefix is not text)
    start = text.index("The multigrid PCG without the host")
    doc = text[start:text.index("int ccp_grid_mg_conjugate_gradient_enqueue(")]
    for word in ("Precondition: ccp_grid_mg_prepare succeeded", "with the same smoothing_sweeps", "CCP_ERR_STATE with nothing enqueued",
                 "4096", "CCP_ERR_BAD_ARG", "no allocation", "no host synchronisation", "EXACTLY max_iteration iterations",
                 "BIT FOR BIT", "being captured", "may NOT be issued during a capture", "the operator setters", "the mask setters",
                 "the mode setters", "the hierarchy kind setter", "It may synchronise", "Calling it twice is harmless",
                 "iterations, [1] converged", "last_l1_step", "b_mean", "x_mean", "reserved", "There is no `seconds`",
                 "ccp_grid_mg_nullspace_info returns CCP_ERR_STATE", "Out of scope", "_rowblocked", "ccp_grid_mg_apply",
                 "relative to |b|", "validation read-back", "the operator is fixed"):
        assert word in doc, word
