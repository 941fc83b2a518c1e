"""CPU: the device hand-off kernels (ccp_grid_io.hpp: k_io_scatter, k_io_gather, k_io_label_check) and the View
instantiations of the assembly, clone, composite and u8 kernels, checked on the gfx950 ISA inside libccp_gs.so like
tests/test_isa_wide.py: every one exists and uses no scratch (private segment 0, no spills).  View is the only accessor:
the host entry points launch the same instantiations on their staging buffers, so no Packed one may come back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("libccp_gs.so or llvm-objdump missing")
    d = tmp_path_factory.mktemp("isa_io")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    out = {}
    for o in objs:
        meta = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        cur = {}
        for line in meta.splitlines():
            m = re.match(r"\s*(-?)\s*\.(\w+):\s+(\S+)", line)
            if not m:
                continue
            item, key, val = m.group(1), m.group(2), m.group(3)
            if item and key == "agpr_count":
                cur = {}
            if key == "name" and val.startswith("_Z"):
                out[val] = cur
            elif key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
                cur[key] = int(val)
    return out


# (kernel name fragment, instantiations expected at least)
KERNELS = [("k_io_scatter", 12), ("k_io_gather", 6), ("k_io_label_check", 1)]
VIEW_KERNELS = ["k_assemble_rhs", "k_assemble_from_images", "k_store_u8", "k_load_u8", "k_blend_field_rhs",
                "k_blend_clone_rhs", "k_blend_composite"]


def _named(notes, frag):
    return {k: v for k, v in notes.items() if frag in k}


@pytest.mark.parametrize("frag,count", KERNELS)
def test_io_kernels_use_no_scratch(notes, frag, count):
    ks = _named(notes, frag)
    assert len(ks) >= count, sorted(ks)
    for name, n in ks.items():
        assert n["private_segment_fixed_size"] == 0, (name, n)
        assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, (name, n)


@pytest.mark.parametrize("frag", VIEW_KERNELS)
def test_view_instantiations_use_no_scratch(notes, frag):
    ks = _named(notes, frag)
    views = {k: v for k, v in ks.items() if "4ViewI" in k}
    assert views, sorted(ks)                                # what the _device twin and the host entry point both launch
    assert not [k for k in notes if "6PackedI" in k]        # no second accessor anywhere in the code object
    for name, n in views.items():
        assert n["private_segment_fixed_size"] == 0, (name, n)
        assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, (name, n)
