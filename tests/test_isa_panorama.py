"""CPU: the kernels of the device mask setter (csrc/ccp_grid_mask.hpp) and of the panorama merge (csrc/ccp_panorama.hpp)
in the BUILT gfx950 code object, from its resource report: every instantiation is there, none spills or uses scratch,
only the erosion uses LDS (its two tiles), and the registers leave at least eight waves per SIMD (<= 64 VGPRs): these
are streaming passes whose loads want many waves in flight."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
EXPECTED = {"k_mask_split": 3, "k_pano_erode": 1, "k_pano_begin": 2, "k_pano_add": 2, "k_pano_finish": 2}
ERODE_LDS = 2 * (16 + 16) * (64 + 16)          # two 0/1 byte tiles of (kErodeTy + 2 * 8) x (kErodeTx + 2 * 8)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_panorama")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    found = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and re.search("|".join(EXPECTED), name.group(1)):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return found


def test_every_instantiation_is_present(kernels):
    for stem, count in EXPECTED.items():
        assert sum(stem in n for n in kernels) == count, (stem, sorted(kernels))


def test_no_spills_no_scratch(kernels):
    assert kernels                                                # an empty report would pass the loop below
    for name, m in sorted(kernels.items()):
        print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name
        assert m["group_segment_fixed_size"] == (ERODE_LDS if "k_pano_erode" in name else 0), name
        assert m["max_flat_workgroup_size"] == 256, name
        assert m["vgpr_count"] <= 64, (name, m["vgpr_count"])
