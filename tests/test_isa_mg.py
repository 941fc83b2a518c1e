"""CPU: the multigrid kernels (csrc/ccp_grid_mg.hpp) in the BUILT gfx950 code object do not spill and the LDS tail fits:
no VGPR/SGPR spills, no scratch, and k_mg_tail's static LDS is its five arrays of kMgTailCells doubles (< 64 KiB)."""
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
    d = tmp_path_factory.mktemp("isa_mg")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_mg_" in name.group(1):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_every_mg_kernel_is_present(mg_kernels):
    for k in ("k_mg_tile", "k_mg_restrict", "k_mg_coarsen", "k_mg_tail", "k_mg_apply", "k_mg_check", "k_mg_beta"):
        assert any(k in n for n in mg_kernels), k


def test_no_spills(mg_kernels):
    for name, m in mg_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_tail_lds(mg_kernels):
    src = open(os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc", "ccp_grid_mg.hpp")).read()
    cells = eval(re.search(r"constexpr int kMgTailCells = ([^;]+);", src).group(1), {"__builtins__": {}})
    tails = [m for n, m in mg_kernels.items() if "k_mg_tail" in n]
    assert tails
    for m in tails:
        assert 5 * 8 * cells <= m["group_segment_fixed_size"] < 64 * 1024
