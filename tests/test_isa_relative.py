"""CPU: the kernels of the relative stop test (k_mgr_* of csrc/ccp_grid_mgr.hpp) in the BUILT gfx950 code objects, read
from the code objects' resource notes alone: each present exactly once over the whole library, no VGPR/SGPR spills, no
scratch, and no LDS beyond the block_sum scratch a kernel declares (kBlock / kWave = 4 doubles; the report kernel
declares none)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
SCRATCH = 4 * 8                                                  # double scratch[kBlock / kWave]
# kernel: the LDS it declares
KERNELS = {"k_mgr_init": SCRATCH, "k_mgr_init_batched": SCRATCH, "k_mgr_init_constant": SCRATCH, "k_mgr_threshold": SCRATCH,
           "k_mgr_threshold_batched": SCRATCH, "k_mgr_check": SCRATCH, "k_mgr_check_batched": SCRATCH, "k_mgr_report": 0}


def base_name(mangled):
    """k_mgr_init of _ZN3ccpL10k_mgr_initEPKdPdS2_lS2_S2_ (the source name stands after its length)"""
    m = re.search(r"\d+(k_mgr_[a-z_]+?)E", mangled)
    return m.group(1) if m else None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_relative")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    found = []
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_mgr_" in name.group(1):
                found.append((name.group(1), {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}))
    return found


def test_each_kernel_is_present_once_and_no_other(kernels):
    names = [base_name(n) for n, _ in kernels]
    assert sorted(names) == sorted(KERNELS), names


def test_no_spills_no_scratch_no_lds_beyond_the_block_sum(kernels):
    assert kernels
    for name, m in kernels:
        print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name
        assert m.get("group_segment_fixed_size", 0) <= KERNELS[base_name(name)], name
