"""CPU: ccp_grid_reserve_constraints and ccp_grid_refresh_constrained_device (include/ccp_gs.h) at the boundary: the header
declares both functions and the library exports them, the header still compiles as C11 and C++17, the ABI version stays 6,
a NULL handle is a bad argument, capi.Grid and tensor_ops.WeightedSolver have the methods with their signatures, and the
header states the contract a caller relies on.  No device is touched."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAMES = ("ccp_grid_reserve_constraints", "ccp_grid_refresh_constrained_device")


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_functions():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    arr = r"const\s+ccp_device_array\s*\*\s*"
    assert re.search(r"int\s+ccp_grid_refresh_constrained_device\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*" + arr + r"wx\s*,\s*" + arr + r"wy\s*,\s*" + arr
                     + r"lambda\s*,\s*" + arr + r"fixed\s*\)\s*;", text)
    assert re.search(r"int\s+ccp_grid_reserve_constraints\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s+on\s*\)\s*;", text)
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive


def test_null_handle_is_a_bad_argument():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    assert lib.ccp_grid_refresh_constrained_device(None, None, None, None, None) == BAD_ARG
    assert lib.ccp_grid_reserve_constraints(None, 1) == BAD_ARG
    assert lib.ccp_grid_reserve_constraints(None, 0) == BAD_ARG


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    ccp_device_array w = {0, CCP_DTYPE_F32, 0, 0, 64, 1, 0};\n"
            "    ccp_device_array m = {0, CCP_DTYPE_U8, 0, 0, 64, 1, 0};\n"
            "    int a = ccp_grid_reserve_constraints(0, 1);\n"
            "    int b = ccp_grid_refresh_constrained_device(0, &w, &w, 0, &m);\n"
            "    return a + b;\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_refresh_mask.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_has_the_two_methods():
    from coursecomputationalphotography_amd import capi
    p = inspect.signature(capi.Grid.reserve_constraints).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    p = inspect.signature(capi.Grid.refresh_constrained_tensor).parameters
    assert list(p) == ["self", "wx", "wy", "lam", "fixed"] and all(p[n].default is None for n in ("wx", "wy", "lam", "fixed"))
    p = inspect.signature(capi.Grid.refresh_weights_tensor).parameters                      # untouched
    assert list(p) == ["self", "wx", "wy", "lam"]


def test_weighted_solver_has_the_two_methods():
    from coursecomputationalphotography_amd import tensor_ops
    assert list(inspect.signature(tensor_ops.WeightedSolver.reserve_constraints).parameters) == ["self"]
    p = inspect.signature(tensor_ops.WeightedSolver.refresh_constraints).parameters
    assert list(p) == ["self", "wx", "wy", "data_weight", "fixed"]
    assert p["wx"].default is inspect.Parameter.empty and p["wy"].default is inspect.Parameter.empty
    assert p["data_weight"].default is None and p["fixed"].default is None
    p = inspect.signature(tensor_ops.WeightedSolver.refresh_operator).parameters             # untouched
    assert list(p) == ["self", "wx", "wy", "data_weight"]
    p = inspect.signature(tensor_ops.WeightedSolver.set_operator).parameters
    assert list(p) == ["self", "wx", "wy", "data_weight", "fixed"]


def test_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*(?!/)", "\n", header()).split())          # (the comment's line prefix is not text)
    start = text.index("Changing the fixed pixels of a weighted operator by enqueue only")
    assert start > text.index("int ccp_grid_refresh_weights_device(")          # the new section follows the refresh section
    doc = text[start:text.index("int ccp_grid_reserve_constraints(")]
    for word in ("sticky flag", "Host state only", "at the next ccp_grid_set_weights_* call", "does not drop an installed operator",
                 "KEEPS the three constraint planes", "even when no pixel is fixed", "equals the unreserved handle's bit for bit",
                 "24 bytes per pixel and set", "or a row block: CCP_ERR_UNSUPPORTED",
                 "NULL is the empty set", "no allocation", "no host synchronisation", "no copy to or from host memory", "no memset",
                 "being captured", "returns CCP_OK", "CCP_OPERATOR_NOT_FLOATING", "poisons the values, never the marks",
                 "Precondition", "the three constraint planes exist", "CCP_ERR_STATE with nothing enqueued",
                 "CCP_ERR_BAD_ARG before anything is enqueued", "Postcondition, bit for bit", "on a fresh reserved handle",
                 "the line smoother's inputs", "the census verdict", "keeps the NEW set", "all three counts of the last refresh that ran",
                 "a replayed one included", "a setter invalidates", "Which planes exist does not change under a refresh",
                 "Out of scope", "the ABI version does not change"):
        assert word in doc, word
