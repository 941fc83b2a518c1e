"""CPU: the batched multigrid kernels (csrc/ccp_grid_mgb.hpp) in the BUILT gfx950 code object: every k_mgb_* kernel is
there, none spills or uses scratch, k_mgb_tail's static LDS is k_mg_tail's (< 64 KiB), and k_mgb_tile's LDS -- no static
LDS in the metadata, the dynamic size the launch asks for (ccp_debug_mgb_tile_lds) -- is at most what NOTES R17.1 states
and fits a CU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_mgb_tile", "k_mgb_restrict", "k_mgb_apply", "k_mgb_tail", "k_mgb_init", "k_mgb_dot", "k_mgb_update",
           "k_mgb_direction", "k_mgb_alpha", "k_mgb_set_rlen", "k_mgb_check", "k_mgb_beta")


@pytest.fixture(scope="module")
def mgb_kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    d = tmp_path_factory.mktemp("isa_mgb")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    kernels = {}
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_mgb_" in name.group(1):
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_every_batched_kernel_is_present(mgb_kernels):
    for k in KERNELS:
        assert any(k in n for n in mgb_kernels), k
    # the tile pass for every level-0 kind, before and after the coarse correction; the product with and without the dot
    assert sum("k_mgb_tile" in n for n in mgb_kernels) == 6
    assert sum("k_mgb_restrict" in n for n in mgb_kernels) == 3
    assert sum("k_mgb_apply" in n for n in mgb_kernels) == 6


def test_no_spills_and_no_scratch(mgb_kernels):
    for k in KERNELS:                                            # an empty report would pass the loop below
        assert any(k in n for n in mgb_kernels), k
    for name, m in mgb_kernels.items():
        assert m.get("vgpr_spill_count", 0) == 0, name
        assert m.get("sgpr_spill_count", 0) == 0, name
        assert m.get("private_segment_fixed_size", 0) == 0, name


def test_tail_lds(mgb_kernels):
    src = open(os.path.join(CSRC, "ccp_grid_mg.hpp")).read()
    cells = eval(re.search(r"constexpr int kMgTailCells = ([^;]+);", src).group(1), {"__builtins__": {}})
    tails = [m for n, m in mgb_kernels.items() if "k_mgb_tail" in n]
    assert len(tails) == 1
    assert 5 * 8 * cells <= tails[0]["group_segment_fixed_size"] < 64 * 1024


def test_tile_lds_is_what_the_notes_state(mgb_kernels):
    tiles = {n: m for n, m in mgb_kernels.items() if "k_mgb_tile" in n}
    for name, m in tiles.items():
        assert m["group_segment_fixed_size"] == 0, name          # all of it is dynamic: mgb_tile_lds
    # the stored-operator kind (template argument 2) runs 1,024 threads, the others 256
    for name, m in tiles.items():
        assert m["max_flat_workgroup_size"] == (1024 if "ILi2E" in name else 256), name
    notes = open(os.path.join(ROOT, "NOTES.md")).read()
    section = notes[notes.index("R17.1"):]
    stated = {int(nu): int(b.replace(",", "")) for nu, b in re.findall(r"nu = (\d): ([\d,]+) B of LDS", section)}
    assert sorted(stated) == [1, 2, 3, 4], stated
    mg = open(os.path.join(CSRC, "ccp_grid_mg.hpp")).read()
    tw, th = (int(v) for v in re.search(r"kMgTileW = (\d+), kMgTileH = (\d+)", mg).groups())
    lib = ctypes.CDLL(LIB)
    lib.ccp_debug_mgb_tile_lds.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    nbytes, threads = ctypes.c_int32(-1), ctypes.c_int32(-1)
    for kind in (0, 1, 2):                                       # structured, mask, stored operator
        for nu in (1, 2, 3, 4):
            assert lib.ccp_debug_mgb_tile_lds(kind, nu, ctypes.byref(nbytes), ctypes.byref(threads)) == 0
            cells = (tw + 4 * nu) * (th + 4 * nu)
            # what the kernel indexes: b and z of one channel, and three fp64 planes or one byte per cell
            assert nbytes.value >= (5 * 8 * cells if kind == 2 else 2 * 8 * cells + cells), (kind, nu, nbytes.value)
            assert threads.value == (1024 if kind == 2 else 256)
            if kind == 2:
                assert nbytes.value <= stated[nu] <= 160 * 1024, (nu, nbytes.value, stated[nu])
            else:
                assert nbytes.value < 64 * 1024, (kind, nu, nbytes.value)    # these kinds stay below the 64 KiB a kernel gets unasked
    for bad in ((-1, 2), (3, 2), (2, 0), (2, 5)):
        assert lib.ccp_debug_mgb_tile_lds(bad[0], bad[1], ctypes.byref(nbytes), ctypes.byref(threads)) == 1
    assert lib.ccp_debug_mgb_tile_lds(2, 2, None, None) == 0
