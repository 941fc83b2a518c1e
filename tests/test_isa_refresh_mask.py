"""CPU: the kernel ccp_grid_refresh_constrained_device adds (k_weighted_fixed_refresh of csrc/ccp_grid_weighted.hpp) in the
BUILT gfx950 code objects, by the resource notes alone: present in exactly one code object, no spills, no scratch, an LDS
tally of three words; and the two operator kernels beside it (k_weighted_coef_fixed, k_weighted_refresh), which the new
one must not have changed: their notes are those of the commit before it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = "k_weighted_fixed_refresh"
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count", "kernarg_segment_size")
# the notes of the two kernels in the build of the commit before k_weighted_fixed_refresh existed (NOTES.md R36.1)
BEFORE = {
    "k_weighted_coef_fixed": dict(vgpr_count=20, sgpr_count=77, agpr_count=0, group_segment_fixed_size=12, private_segment_fixed_size=0,
                                  vgpr_spill_count=0, sgpr_spill_count=0, kernarg_segment_size=256),
    "k_weighted_refresh": dict(vgpr_count=26, sgpr_count=72, agpr_count=0, group_segment_fixed_size=8, private_segment_fixed_size=0,
                               vgpr_spill_count=0, sgpr_spill_count=0, kernarg_segment_size=208),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_refresh_mask")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    found = []
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_weighted_" in name.group(1):
                m = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
                m["agpr_count"] = int(re.match(r":\s+(\d+)", block).group(1))
                found.append((o, name.group(1), m))
    return found


def named(kernels, kernel):
    """the kernels whose mangled name holds `kernel` as a whole identifier (k_weighted_refresh is no k_weighted_fixed_refresh)"""
    return [(o, n, m) for o, n, m in kernels if re.search(rf"\d{kernel}(?![a-z_])", n)]


def test_the_new_kernel_is_in_exactly_one_code_object(kernels):
    assert len(named(kernels, NEW)) == 1, [n for _, n, _ in kernels]


def test_no_spills_no_scratch_and_a_three_word_tally(kernels):
    (_, name, m), = named(kernels, NEW)
    print(name, {k: m.get(k) for k in FIELDS})
    assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0
    assert m.get("private_segment_fixed_size", 0) == 0
    assert m.get("group_segment_fixed_size", 0) == 12


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_the_kernels_beside_it_are_what_they_were(kernels, kernel):
    found = named(kernels, kernel)
    assert len(found) == 1, (kernel, [n for _, n, _ in kernels])
    got = {k: found[0][2].get(k, 0) for k in FIELDS}
    assert got == BEFORE[kernel], (kernel, got)
