"""CPU: the wide-strip depth-8 kernel (ccp_grid_fused_wide.hpp, k_fused_sweep_wide), checked on the gfx950 ISA inside
libccp_gs.so like tests/test_isa_red_skip.py.

1. One wavefront is one worker: no s_barrier, and the march never touches scratch (no spills of either kind).
2. Registers: at most 256 architectural VGPRs; the few AGPRs it uses (occupancy is one wave per SIMD, set by its LDS
   ring, so they cost no occupancy) stay few.
3. Memory: x and b move as 16-byte pairs (dwordx4, never dwordx2), no more loads per row than the 128-px kernel but
   for 224 stored pixels instead of 96 — under half the load instructions per stored pixel — and b is read from LDS.
4. Both store forms exist and the !STORE_RED form issues half the stores.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"
WIDE = {True: "_ZN3ccp18k_fused_sweep_wideILi8ELb1EEEvNS_11FusedParamsEiii",
        False: "_ZN3ccp18k_fused_sweep_wideILi8ELb0EEEvNS_11FusedParamsEiii"}
NARROW = "_ZN3ccp13k_fused_sweepILi8ELi0ELi2ELb0ELb0EEEvNS_11FusedParamsE"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("libccp_gs.so or llvm-objdump missing")
    d = tmp_path_factory.mktemp("isa_wide")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    functions, notes = {}, {}
    for o in objs:
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", o], check=True, capture_output=True, text=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if m:
                name = m.group(1)
                functions[name] = []
            elif name and line.startswith("\t"):
                functions[name].append(line.split("//")[0].strip())
        meta = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        cur = {}
        for line in meta.splitlines():
            m = re.match(r"\s*(-?)\s*\.(\w+):\s+(\S+)", line)
            if not m:
                continue
            item, key, val = m.group(1), m.group(2), m.group(3)
            if item and key == "agpr_count":                     # each kernel's record is a list item starting here
                cur = {}
            if key == "name" and val.startswith("_Z"):
                notes[val] = cur
            elif key in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                         "group_segment_fixed_size"):
                cur[key] = int(val)
    return functions, notes


def _count(body, prefix):
    return sum(1 for ins in body if ins.startswith(prefix))


@pytest.mark.parametrize("store_red", [True, False])
def test_wide_budget(isa, store_red):
    functions, notes = isa
    n = notes[WIDE[store_red]]
    assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, n
    assert n["private_segment_fixed_size"] == 0, n
    assert n["vgpr_count"] - n["agpr_count"] <= 256 and n["agpr_count"] <= 32, n
    assert n["group_segment_fixed_size"] <= 160 * 1024, n
    body = functions[WIDE[store_red]]
    assert _count(body, "s_barrier") == 0
    assert _count(body, "scratch_") == 0 and _count(body, "buffer_store_dword v") == 0


@pytest.mark.parametrize("store_red", [True, False])
def test_wide_moves_pairs(isa, store_red):
    functions, _ = isa
    body = functions[WIDE[store_red]]
    assert _count(body, "buffer_load_dwordx2") == 0 and _count(body, "buffer_store_dwordx2") == 0
    loads, stores = _count(body, "buffer_load_dwordx4"), _count(body, "buffer_store_dwordx4")
    # per row: x black, b red, b black (a loaded row's red x is recomputed by half-sweep 1 before anything reads it, so
    # the compiler leaves its load out)
    assert loads > 0 and loads % 3 == 0
    reads = _count(body, "ds_read_b128")
    assert reads == 16 * stores // (2 if store_red else 1)      # one b pair per half-sweep, 2T per stored row


def test_wide_half_the_stores_without_red(isa):
    functions, _ = isa
    full, skip = (_count(functions[WIDE[s]], "buffer_store_dwordx4") for s in (True, False))
    assert full > 0 and skip * 2 == full


def test_wide_loads_per_stored_pixel(isa):
    """Per march step both kernels load one row; the wide one stores 224 pixels of it, the narrow 96."""
    functions, _ = isa
    wide, narrow = functions[WIDE[False]], functions[NARROW]
    per_step_wide = _count(wide, "buffer_load_dwordx4") / _count(wide, "buffer_store_dwordx4")
    per_step_narrow = _count(narrow, "buffer_load_dwordx2") / _count(narrow, "buffer_store_dwordx2")
    assert per_step_wide <= per_step_narrow
    assert (per_step_wide / 224) <= 0.5 * (per_step_narrow / 96)
