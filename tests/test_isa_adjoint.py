"""CPU: the backward pass's kernels (csrc/ccp_grid_adjoint.hpp) in the BUILT gfx950 code object, from its resource report:
k_weighted_adjoint and k_adjoint_begin are there, neither spills nor uses scratch, neither uses LDS (the neighbours come
from the cache), and the vector registers leave at least five waves per SIMD (<= 96 of 512 VGPRs per lane: twenty waves
per CU keep the loads of a bandwidth-bound pass in flight)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def adjoint_kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_adjoint")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and re.search(r"k_weighted_adjoint|k_adjoint_begin", name.group(1)):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_both_kernels_are_present(adjoint_kernels):
    assert sum("k_weighted_adjoint" in n for n in adjoint_kernels) == 1, sorted(adjoint_kernels)
    assert sum("k_adjoint_begin" in n for n in adjoint_kernels) == 1, sorted(adjoint_kernels)


def test_no_spills_no_scratch_no_lds(adjoint_kernels):
    assert adjoint_kernels                                        # an empty report would pass the loop below
    for name, m in adjoint_kernels.items():
        print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name
        assert m["group_segment_fixed_size"] == 0, name
        assert m["max_flat_workgroup_size"] == 256, name
        assert m["vgpr_count"] <= 96, (name, m["vgpr_count"])
