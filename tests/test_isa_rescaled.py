"""CPU: the multigrid kernels after the correction scale and the coarsening's edge factor became kernel arguments
(csrc/ccp_grid_mg.hpp; CCP_MG_HIERARCHY_RESCALED), in the BUILT gfx950 code object: every k_mg_* kernel still has no
VGPR/SGPR spills and no scratch, k_mg_tail's static LDS is still exactly its five arrays of kMgTailCells doubles, and
the weighted coarsening (k_weighted_coarsen, which serves the shared operator and the per-channel ones) is there once (the
edge factor is an argument, not a template parameter)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def mg_kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_rescaled")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and ("k_mg_" in name.group(1) or "k_weighted_coarsen" in name.group(1)):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_kernels_present(mg_kernels):
    assert sum(1 for n in mg_kernels if "k_weighted_coarsen" in n) == 1
    assert sum(1 for n in mg_kernels if "k_mg_tail" in n) == 1
    # k_mg_tile: three operator kinds x (pre, post)
    assert sum(1 for n in mg_kernels if "k_mg_tile" in n) == 6


def test_no_spills_no_scratch(mg_kernels):
    assert mg_kernels
    for name, m in mg_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_tail_lds_is_its_five_arrays(mg_kernels):
    src = open(os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc", "ccp_grid_mg.hpp")).read()
    cells = eval(re.search(r"constexpr int kMgTailCells = ([^;]+);", src).group(1), {"__builtins__": {}})
    assert cells == 1365
    (tail,) = [m for n, m in mg_kernels.items() if "k_mg_tail" in n]
    # five arrays of `cells` doubles, each placed on a 16-byte boundary: nothing was added for the scale
    assert tail["group_segment_fixed_size"] == 4 * ((8 * cells + 15) // 16 * 16) + 8 * cells
