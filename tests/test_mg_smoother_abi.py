"""CPU: the smoother choice of the multigrid PCG (include/ccp_gs.h, ccp_grid_mg_set_smoother / _get_smoother) at the
boundary: the header declares both functions and the library exports them, a NULL handle is a bad argument, the header
still compiles as C11 and C++17, capi refuses an unknown name, and the header documents the refusals and what
smoothing_sweeps 0 means in either mode.  No device is touched."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAMES = ("ccp_grid_mg_set_smoother", "ccp_grid_mg_get_smoother")


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_two_functions():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+ccp_grid_mg_set_smoother\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s+kind\s*\)\s*;", text)
    assert re.search(r"int\s+ccp_grid_mg_get_smoother\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s*\*\s*kind\s*\)\s*;", text)
    assert re.search(r"#define\s+CCP_MG_SMOOTHER_POINT\s+0\b", text) and re.search(r"#define\s+CCP_MG_SMOOTHER_LINE\s+1\b", text)
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6                            # additive, as the precision and channels setters were


def test_header_documents_the_refusals_and_the_sweep_default():
    text = " ".join(header().split())
    start = text.index("The smoother of the V-cycle of ccp_grid_mg_conjugate_gradient and ccp_grid_mg_apply")
    doc = text[start:text.index("#define CCP_MG_SMOOTHER_POINT")]
    for word in ("structured handle", "Dirichlet-mask handle", "CCP_MG_PRECISION_F32", "CCP_MG_CHANNELS_BATCHED", "_rowblocked",
                 "CCP_ERR_UNSUPPORTED", "x and b untouched"):
        assert word in doc, word
    assert "the value 0 means the smoother's default, 2 sweeps in POINT mode and 1 sweep in LINE mode" in doc
    assert "without pivoting" in doc and "identity row" in doc
    assert "24 B" in doc                                         # the work planes


def test_null_handle_is_a_bad_argument():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    value = ctypes.c_int32(-1)
    assert lib.ccp_grid_mg_set_smoother(None, 1) == BAD_ARG
    assert lib.ccp_grid_mg_set_smoother(None, 0) == BAD_ARG
    assert lib.ccp_grid_mg_get_smoother(None, ctypes.byref(value)) == BAD_ARG
    assert lib.ccp_grid_mg_get_smoother(None, None) == BAD_ARG
    assert value.value == -1


def test_header_compiles_as_c11_and_cxx17_and_the_constants_are_usable(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    int32_t kind = CCP_MG_SMOOTHER_POINT;\n"
            "    int a = ccp_grid_mg_set_smoother(0, CCP_MG_SMOOTHER_LINE);\n"
            "    int b = ccp_grid_mg_get_smoother(0, &kind);\n"
            "    return a + b + (int)kind;\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_smoother.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "use_facade.cc"
    src.write_text('#include "ccp/photomontage.h"\n'
                   "static_assert((int)ccp::Smoother::Point == 0 && (int)ccp::Smoother::Line == 1, \"Smoother\");\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_rejects_an_unknown_name():
    from coursecomputationalphotography_amd import capi
    assert capi.MG_SMOOTHERS == {"point": 0, "line": 1}
    assert capi.mg_smoother_value("point") == 0 and capi.mg_smoother_value("line") == 1
    assert capi.mg_smoother_value(1) == 1
    for bad in ("zebra", "", "Line", 2, -1):
        with pytest.raises(ValueError):
            capi.mg_smoother_value(bad)
    assert hasattr(capi.Grid, "mg_set_smoother") and hasattr(capi.Grid, "mg_smoother")


def test_tensor_ops_take_the_keyword():
    from coursecomputationalphotography_amd import tensor_ops
    for name in ("weighted_solve", "wls_smooth", "constrained_solve", "seamless_clone_constrained"):
        p = inspect.signature(getattr(tensor_ops, name)).parameters
        assert "smoother" in p and p["smoother"].default == "point", name
