"""CPU: ccp_grid_refresh_weights_device and ccp_grid_operator_status (include/ccp_gs.h) at the boundary: the header
declares both functions and the three status macros and the library exports them, the header still compiles as C11 and
C++17, the ABI version stays 6, a NULL handle is a bad argument, capi.Grid and tensor_ops.WeightedSolver have the
methods with their signatures, and the header states the contract a caller relies on.  No device is touched."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAMES = ("ccp_grid_refresh_weights_device", "ccp_grid_operator_status")


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_functions():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    arr = r"const\s+ccp_device_array\s*\*\s*"
    assert re.search(r"int\s+ccp_grid_refresh_weights_device\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*" + arr + r"wx\s*,\s*" + arr + r"wy\s*,\s*" + arr
                     + r"lambda\s*\)\s*;", text)
    assert re.search(r"int\s+ccp_grid_operator_status\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s*\*\s*status\s*\)\s*;", text)
    for macro, value in (("CCP_OPERATOR_BAD_WEIGHT", 1), ("CCP_OPERATOR_F32_RANGE", 2), ("CCP_OPERATOR_NOT_FLOATING", 4)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", text), macro
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive


def test_null_handle_is_a_bad_argument():
    import ctypes as C
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    assert lib.ccp_grid_refresh_weights_device(None, None, None, None) == BAD_ARG
    word = C.c_int32(-3)
    assert lib.ccp_grid_operator_status(None, C.byref(word)) == BAD_ARG
    assert lib.ccp_grid_operator_status(None, None) == BAD_ARG
    assert word.value == -3


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    ccp_device_array w = {0, CCP_DTYPE_F32, 0, 0, 64, 1, 0};\n"
            "    int32_t status = CCP_OPERATOR_BAD_WEIGHT | CCP_OPERATOR_F32_RANGE | CCP_OPERATOR_NOT_FLOATING;\n"
            "    int a = ccp_grid_refresh_weights_device(0, &w, &w, 0);\n"
            "    int b = ccp_grid_operator_status(0, &status);\n"
            "    return a + b + (status == 7 ? 0 : 1);\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_refresh.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_has_the_two_methods():
    from coursecomputationalphotography_amd import capi
    p = inspect.signature(capi.Grid.refresh_weights_tensor).parameters
    assert list(p) == ["self", "wx", "wy", "lam"] and all(p[n].default is None for n in ("wx", "wy", "lam"))
    assert list(inspect.signature(capi.Grid.operator_status).parameters) == ["self"]


def test_weighted_solver_has_the_refresh_and_the_weight_keywords():
    from coursecomputationalphotography_amd import tensor_ops
    p = inspect.signature(tensor_ops.WeightedSolver.refresh_operator).parameters
    assert list(p) == ["self", "wx", "wy", "data_weight"] and p["data_weight"].default is None
    assert p["wx"].default is inspect.Parameter.empty and p["wy"].default is inspect.Parameter.empty
    p = inspect.signature(tensor_ops.WeightedSolver.solve_grad).parameters
    assert list(p) == ["self", "gx", "gy", "f", "values", "x0", "report", "adjoint_report", "wx", "wy", "data_weight"]
    for name in ("wx", "wy", "data_weight"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None, name
    p = inspect.signature(tensor_ops.WeightedSolver.set_operator).parameters               # still the call that takes `fixed`
    assert list(p) == ["self", "wx", "wy", "data_weight", "fixed"]


def test_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*(?!/)", "\n", header()).split())          # (the comment's line prefix is not text)
    start = text.index("Refreshing a weighted operator by enqueue only")
    assert start > text.index("int ccp_grid_mg_conjugate_gradient_enqueue(")   # the new section follows that declaration
    doc = text[start:text.index("int ccp_grid_refresh_weights_device(")]
    for word in ("no allocation", "no host synchronisation", "no copy to or from host", "being captured", "the set of fixed pixels",
                 "whether the three constraint planes exist", "the hierarchy kind and every mode", "stays prepared", "bit for bit",
                 "ccp_grid_set_weights_constrained_device", "ccp_grid_set_weights_per_channel_device", "Precondition",
                 "CCP_ERR_STATE with nothing enqueued", "CCP_ERR_BAD_ARG before anything is enqueued", "CCP_ERR_UNSUPPORTED",
                 "returns CCP_OK", "CCP_OPERATOR_BAD_WEIGHT (1)", "CCP_OPERATOR_F32_RANGE (2)", "CCP_OPERATOR_NOT_FLOATING (4)",
                 "starts every channel stopped", "untouched bit for bit", "iterations 0, converged 0 and [5] = the status",
                 "poisoned, not dropped", "restores it fully", "ccp_grid_operator_status synchronises",
                 "ccp_grid_mg_conjugate_gradient, ccp_grid_mg_apply and ccp_grid_mg_prepare read the word first", "read back on demand",
                 "Out of scope", "the ABI version does not change"):
        assert word in doc, word
