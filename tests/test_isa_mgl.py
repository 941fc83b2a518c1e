"""CPU: the line-smoother kernels (csrc/ccp_grid_mgl.hpp) in the BUILT gfx950 code object, from its resource report:
every k_mgl_lines instance is there, none spills or uses scratch, and their LDS -- all static, the launches ask for no
dynamic LDS -- is kMglLdsBytes (24,576 B), within the 64 KiB a kernel gets unasked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def mgl_kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_mgl")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_mgl_" in name.group(1):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_every_line_kernel_is_present(mgl_kernels):
    # rows: from b alone and from z; columns: from z and with the prolongation fused
    assert sum("k_mgl_lines" in n for n in mgl_kernels) == 4, sorted(mgl_kernels)


def test_no_spills_and_no_scratch(mgl_kernels):
    assert mgl_kernels                                            # an empty report would pass the loop below
    for name, m in mgl_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_lds_is_static_and_within_a_kernels_default(mgl_kernels):
    lds = 12 * 256 * 8                                           # kMglLdsBytes: twelve planes of 256 doubles, all static
    assert mgl_kernels
    for name, m in mgl_kernels.items():
        assert m["group_segment_fixed_size"] == lds < 64 * 1024, (name, m["group_segment_fixed_size"])
        assert m["max_flat_workgroup_size"] == 256, name
