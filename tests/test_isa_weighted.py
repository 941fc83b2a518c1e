"""CPU: the weighted-grid kernels (csrc/ccp_grid_weighted.hpp, k_weighted_coarsen in csrc/ccp_grid_mg.hpp, and the
stored-operator instantiations of the multigrid kernels a weighted handle runs on level 0) in the BUILT gfx950 code
objects: all present, the operator kernels in their exact numbers over the whole library and each in one code object,
no VGPR/SGPR spills, no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
OPERATOR = ("k_weighted_coef", "k_weighted_rhs", "k_weighted_coarsen")   # (k_weighted_coef_fixed has the first as a substring)
NAMES = ("k_weighted_coef", "k_weighted_rhs", "k_weighted_apply", "k_weighted_coarsen", "k_mg_apply", "k_mg_tile")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_weighted")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    found = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and any(n in name.group(1) for n in NAMES + ("k_mg_coarsen_weighted",)):
                if any(n in name.group(1) for n in OPERATOR):
                    assert name.group(1) not in found, f"{name.group(1)} is in two code objects"
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return found


def test_every_weighted_kernel_is_present(kernels):
    for k in NAMES[:4]:
        assert any(k in n for n in kernels), k
    # the multigrid kernels on a stored level-0 operator: kind kMgCoarse (= 2) of the PCG product, with and without dot
    assert sum(1 for n in kernels if "k_mg_apply" in n and "ILi2E" in n) == 2


def test_one_operator_kernel_family(kernels):
    """The formation, the right-hand side and the coarsening exist once for the shared operator and the per-channel ones:
    INIT x FIXED right-hand sides, the formation with and without a mask, one coarsening, none left of the templates
    over View<T> or of the shared operator's own coarsening kernel."""
    assert sum(1 for n in kernels if "k_weighted_rhs" in n) == 4
    assert sum(1 for n in kernels if "k_weighted_coef" in n) == 2
    assert sum(1 for n in kernels if "k_weighted_coarsen" in n) == 1
    assert not [n for n in kernels if "k_weighted_rhs" in n and "4ViewI" in n]
    assert not [n for n in kernels if "k_mg_coarsen_weighted" in n]


def test_no_spills_no_scratch(kernels):
    for name, m in kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name
