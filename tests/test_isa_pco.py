"""CPU: the kernels behind the launchers of csrc/ccp_grid_weighted.hip in the BUILT gfx950 code objects: the weighted
handle's operator kernels, which serve one operator and one per channel alike (csrc/ccp_grid_weighted.hpp:
k_weighted_coef, k_weighted_coef_fixed, k_weighted_rhs; csrc/ccp_grid_mg.hpp: k_weighted_coarsen), and the per-channel
batched mode's k_pco_* (csrc/ccp_grid_pco.hpp).  Every one is there, in exactly one code object, none spills or uses
scratch, no kernel of the templates they replaced is left, k_pco_tile has no static LDS (all of it is dynamic:
mgb_tile_lds(kMgCoarse, nu)) and runs 1,024 threads, and k_pco_tail's static LDS is k_mg_tail's (< 64 KiB).  Resource
metadata only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
OPERATOR = ("k_weighted_coef", "k_weighted_coef_fixed", "k_weighted_rhs", "k_weighted_coarsen")
KERNELS = OPERATOR + ("k_pco_tile", "k_pco_restrict", "k_pco_apply", "k_pco_tail")


@pytest.fixture(scope="module")
def all_kernels(tmp_path_factory):
    """every kernel of the library: name -> metadata; a name met in two code objects fails here"""
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_pco")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and name.group(1).startswith("_Z"):
                if any(k in name.group(1) for k in KERNELS):
                    assert name.group(1) not in kernels, f"{name.group(1)} is in two code objects"
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


@pytest.fixture(scope="module")
def pco_kernels(all_kernels):
    return {n: m for n, m in all_kernels.items() if any(k in n for k in KERNELS)}


def test_every_kernel_is_present_once(pco_kernels):
    for k in KERNELS:
        assert any(k in n for n in pco_kernels), k
    # before and after the coarse correction; the product with and without the dot; b with and without init and fixed pixels
    assert sum("k_pco_tile" in n for n in pco_kernels) == 2
    assert sum("k_pco_apply" in n for n in pco_kernels) == 2
    assert sum("k_weighted_rhs" in n for n in pco_kernels) == 4
    assert sum("k_weighted_coef" in n for n in pco_kernels) == 2      # k_weighted_coef and k_weighted_coef_fixed
    assert sum("k_weighted_coarsen" in n for n in pco_kernels) == 1


def test_no_kernel_of_the_old_templates_survives(all_kernels):
    """Over the whole library: the right-hand side no longer takes View<T> accessors, and the shared operator has no
    coarsening kernel of its own."""
    assert all_kernels
    assert not [n for n in all_kernels if "k_weighted_rhs" in n and "4ViewI" in n]
    assert not [n for n in all_kernels if "k_mg_coarsen_weighted" in n]
    assert not [n for n in all_kernels if any(k in n for k in ("k_pco_coef", "k_pco_rhs", "k_pco_coarsen"))]


def test_no_spills_and_no_scratch(pco_kernels):
    for k in KERNELS:                                            # an empty report would pass the loop below
        assert any(k in n for n in pco_kernels), k
    for name, m in pco_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_tile_lds_is_dynamic_and_tail_lds_is_the_sequential_tails(pco_kernels):
    tiles = {n: m for n, m in pco_kernels.items() if "k_pco_tile" in n}
    for name, m in tiles.items():
        assert m["group_segment_fixed_size"] == 0, name
        assert m["max_flat_workgroup_size"] == 1024, name
    src = open(os.path.join(CSRC, "ccp_grid_mg.hpp")).read()
    cells = eval(re.search(r"constexpr int kMgTailCells = ([^;]+);", src).group(1), {"__builtins__": {}})
    tails = [m for n, m in pco_kernels.items() if "k_pco_tail" in n]
    assert len(tails) == 1
    assert 5 * 8 * cells <= tails[0]["group_segment_fixed_size"] < 64 * 1024


def test_the_names_touch_no_other_kernel_family():
    """The ISA tests of the existing kernels count instantiations by substring."""
    for k in KERNELS:
        for family in ("k_mg_", "k_mgb_", "k_mgs_", "k_mgl_", "k_weighted_apply", "k_weighted_count_dead", "k_weighted_adjoint",
                       "k_adjoint_begin"):
            assert family not in k
