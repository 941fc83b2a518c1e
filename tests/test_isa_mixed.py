"""CPU: the fp32 V-cycle's kernels (csrc/ccp_grid_mgs.hpp) in the BUILT gfx950 code object: every k_mgs_* kernel is there
(the narrowing pass, the tile pass for every level kind and direction, the restriction, the tail), none has VGPR or SGPR
spills or scratch, and the tail's static LDS is exactly its five arrays of kMgTailCells floats."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def mgs_kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_mixed")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_mgs_" in name.group(1):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_every_fp32_kernel_is_present(mgs_kernels):
    count = {k: sum(1 for n in mgs_kernels if k in n) for k in ("k_mgs_narrow", "k_mgs_tile", "k_mgs_restrict", "k_mgs_tail")}
    # tile: level 0 of three kinds x (pre-smoothing to t, post-smoothing to the PCG's z, the 1x1 image's one pass) + the coarse
    # levels' two; restrict: level 0 of three kinds + the coarse levels'
    assert count == {"k_mgs_narrow": 1, "k_mgs_tile": 11, "k_mgs_restrict": 4, "k_mgs_tail": 1}, count
    assert not any("k_mg_" in n for n in mgs_kernels)        # the fp64 kernels' tests count names that contain k_mg_


def test_no_spills_no_scratch(mgs_kernels):
    assert mgs_kernels
    for name, m in mgs_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_tail_lds_is_its_five_float_arrays(mgs_kernels):
    src = open(os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc", "ccp_grid_mg.hpp")).read()
    cells = eval(re.search(r"constexpr int kMgTailCells = ([^;]+);", src).group(1), {"__builtins__": {}})
    assert cells == 1365
    (tail,) = [m for n, m in mgs_kernels.items() if "k_mgs_tail" in n]
    # five arrays of `cells` floats, each placed on a 16-byte boundary
    assert tail["group_segment_fixed_size"] == 4 * ((4 * cells + 15) // 16 * 16) + 4 * cells
