"""CPU: the channel mode of the multigrid PCG (include/ccp_gs.h, ccp_grid_mg_set_channels / _get_channels) at the
boundary: the header declares both functions and the library exports them, a NULL handle is a bad argument, the header
still compiles as C11 and C++17, and the Python layers refuse an unknown mode and a solver the mode does not apply to.
No device is touched."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BAD_ARG = 1
NAMES = ("ccp_grid_mg_set_channels", "ccp_grid_mg_get_channels")


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_and_library_exports_the_two_functions():
    from coursecomputationalphotography_amd import capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+ccp_grid_mg_set_channels\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s+mode\s*\)\s*;", text)
    assert re.search(r"int\s+ccp_grid_mg_get_channels\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*int32_t\s*\*\s*mode\s*\)\s*;", text)
    assert re.search(r"#define\s+CCP_MG_CHANNELS_SEQUENTIAL\s+0\b", text) and re.search(r"#define\s+CCP_MG_CHANNELS_BATCHED\s+1\b", text)
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6


def test_header_documents_the_refusals_and_the_seconds_field():
    text = " ".join(header().split())
    start = text.index("How ccp_grid_mg_conjugate_gradient and ccp_grid_mg_apply go through the channels")
    doc = text[start:text.index("#define CCP_MG_CHANNELS_SEQUENTIAL")]
    assert "CCP_MG_PRECISION_F32" in doc and "_rowblocked" in doc and "CCP_ERR_UNSUPPORTED" in doc
    assert "seconds" in doc and "whole batched solve" in doc


def test_null_handle_is_a_bad_argument():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    value = ctypes.c_int32(-1)
    assert lib.ccp_grid_mg_set_channels(None, 1) == BAD_ARG
    assert lib.ccp_grid_mg_set_channels(None, 0) == BAD_ARG
    assert lib.ccp_grid_mg_get_channels(None, ctypes.byref(value)) == BAD_ARG
    assert lib.ccp_grid_mg_get_channels(None, None) == BAD_ARG
    assert value.value == -1


def test_header_compiles_as_c11_and_cxx17_and_the_constants_are_usable(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ('#include "ccp_gs.h"\n'
            "int main(void) {\n"
            "    int32_t mode = CCP_MG_CHANNELS_SEQUENTIAL;\n"
            "    int a = ccp_grid_mg_set_channels(0, CCP_MG_CHANNELS_BATCHED);\n"
            "    int b = ccp_grid_mg_get_channels(0, &mode);\n"
            "    return a + b + (int)mode;\n"
            "}\n")
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cc")):
        if shutil.which(cc) is None:
            pytest.skip(f"no {cc}")
        src = tmp_path / f"use_channels.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(src)])
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "use_facade.cc"
    src.write_text('#include "ccp/photomontage.h"\n'
                   "static_assert((int)ccp::Channels::Sequential == 0 && (int)ccp::Channels::Batched == 1, \"Channels\");\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)])


def test_capi_rejects_an_unknown_mode():
    from coursecomputationalphotography_amd import capi
    assert capi.MG_CHANNELS == {"sequential": 0, "batched": 1}
    assert capi.mg_channels_value("sequential") == 0 and capi.mg_channels_value("batched") == 1
    assert capi.mg_channels_value(1) == 1
    for bad in ("interleaved", "", "Batched", 2, -1):
        with pytest.raises(ValueError):
            capi.mg_channels_value(bad)
    assert hasattr(capi.Grid, "mg_set_channels") and hasattr(capi.Grid, "mg_channels")


def test_tensor_ops_refuse_batched_with_another_solver():
    import inspect

    import torch

    from coursecomputationalphotography_amd import tensor_ops
    gx = torch.zeros(4, 4, 3)
    for solver in ("GaussSeidel", "ConjugateGradient"):
        with pytest.raises(ValueError, match="channels"):
            tensor_ops.solve_channels(gx, gx, [3, 3, 3], 5, solver=solver, channels="batched")
    for fn in (tensor_ops.solve_channels, tensor_ops.weighted_solve, tensor_ops.wls_smooth, tensor_ops.constrained_solve,
               tensor_ops.seamless_clone_constrained):
        assert inspect.signature(fn).parameters["channels"].default == "sequential", fn.__name__
