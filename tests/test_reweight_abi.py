"""CPU: ccp_grid_reweight_device at the boundary: the header declares the call, its struct and its constants, the library
exports it, capi binds it with the struct's layout, and the names are checked before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header():
    return open(os.path.join(ROOT, "include", "ccp_gs.h")).read()


def test_header_declares_the_call_and_the_constants():
    text = header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+ccp_grid_reweight_device\s*\(\s*ccp_grid\s*\*\s*g\s*,\s*const\s+ccp_reweight\s*\*\s*how\s*\)\s*;", code)
    want = {"CCP_REWEIGHT_CHARBONNIER": 0, "CCP_REWEIGHT_HUBER": 1, "CCP_REWEIGHT_RECIPROCAL": 2, "CCP_REWEIGHT_EDGE": 0, "CCP_REWEIGHT_PIXEL": 1}
    for name, value in want.items():
        m = re.search(rf"#define\s+{name}\s+(\d+)", code)
        assert m and int(m.group(1)) == value, name
    struct = re.search(r"typedef\s+struct\s+ccp_reweight\s*\{(.*?)\}\s*ccp_reweight\s*;", code, flags=re.S)
    assert struct
    fields = re.findall(r"\*?\s*([a-z_]+)\s*[,;]", struct.group(1))
    assert fields == ["penalty", "coupling", "scale", "epsilon", "u", "gx", "gy", "base_wx", "base_wy", "lambda", "out_wx", "out_wy"], fields
    # the section fixes the operation order and says what it leaves out
    section = text[text.index("Reweighting a weighted operator from the solution"):text.index("#define CCP_REWEIGHT_CHARBONNIER")]
    for phrase in ("acc += r * r", "t = scale * phi(q)", "w = base * t", "q_x + q_y", "Out of scope", "ABI version does not change"):
        assert phrase in section, phrase


def test_library_exports_it_and_capi_binds_it():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    assert hasattr(lib, "ccp_grid_reweight_device")
    assert "ccp_grid_reweight_device" in capi.ABI_SYMBOLS
    assert lib.ccp_abi_version() == 6
    assert lib.ccp_grid_reweight_device.argtypes[1]._type_ is capi.Reweight
    names = [n for n, _ in capi.Reweight._fields_]
    assert names == ["penalty", "coupling", "scale", "epsilon"] + list(capi.REWEIGHT_VIEWS)
    assert capi.Reweight.scale.offset == 8 and capi.Reweight.epsilon.offset == 16 and capi.Reweight.u.offset == 24
    assert C.sizeof(capi.Reweight) == 24 + 8 * C.sizeof(C.c_void_p)
    assert capi.REWEIGHT_PENALTIES == {"charbonnier": 0, "huber": 1, "reciprocal": 2}
    assert capi.REWEIGHT_COUPLINGS == {"edge": 0, "pixel": 1}
    assert hasattr(capi.Grid, "reweight_tensor")


def test_a_null_handle_is_refused_before_the_device():
    from coursecomputationalphotography_amd import capi
    lib = capi.load()
    how = capi.Reweight(0, 0, 1.0, 1e-2)
    assert lib.ccp_grid_reweight_device(None, C.byref(how)) == 1
    assert lib.ccp_grid_reweight_device(None, None) == 1


def test_unknown_names_raise_before_any_device_is_touched():
    from coursecomputationalphotography_amd import capi, tensor_ops
    for penalty, coupling in (("l1", "edge"), ("huber", "isotropic"), (0, "edge"), ("charbonnier", None)):
        with pytest.raises(ValueError):
            capi.reweight_ids(penalty, coupling)
        # a Grid that was never created: the names are looked at before self is
        with pytest.raises(ValueError):
            capi.Grid.reweight_tensor(object(), penalty, coupling, 1.0, 1e-2)
        with pytest.raises(ValueError):
            tensor_ops.irls_solve(None, None, None, 2, 10, penalty=penalty, coupling=coupling)
    assert capi.reweight_ids("reciprocal", "pixel") == (2, 1)
    for name in ("irls_solve", "tv_denoise"):
        assert callable(getattr(tensor_ops, name))
    assert hasattr(tensor_ops.WeightedSolver, "reweight")
