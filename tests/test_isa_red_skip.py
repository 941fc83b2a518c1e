"""CPU: the ordinary-tile kernels built to leave out the red half-row store (STORE_RED = false, ccp_grid_fused.hpp's
fused_wave) — checked on the gfx950 ISA inside libccp_gs.so, like tests/test_isa_invariants.py.

1. The instantiation really issues half the x stores of its full-store twin: the store is left out, not dropped at run time
   by the range check (that form still counts in vmcnt, which the march's loads wait on).
2. It keeps the register budget of the depth-8 pass: <= 256 VGPRs, no vector or scalar spills.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("libccp_gs.so or llvm-objdump missing")
    d = tmp_path_factory.mktemp("isa_red")
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
            m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name" and m.group(2).startswith("_Z"):
                cur = notes.setdefault(m.group(2), cur if "name" not in cur else {})
                cur["name"] = m.group(2)
            elif m.group(1) in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count"):
                cur[m.group(1)] = int(m.group(2))
    return functions, notes


def _one(functions, pattern):
    hits = [n for n in functions if re.search(pattern, n)]
    assert len(hits) == 1, (pattern, hits)
    return hits[0]


def _stores(body):
    return sum(1 for ins in body if ins.startswith("buffer_store_dwordx2"))


# (kernel, template arguments of the full-store form, the same with STORE_RED = false)
KERNELS = [("k_fused_sweep", "ILi%dELi0ELi2ELb0ELb1EEEv", "ILi%dELi0ELi2ELb0ELb0EEEv"),
           ("k_fused_sweep_masked", "ILi%dELi0ELi2ELb1EEEv", "ILi%dELi0ELi2ELb0EEEv")]


@pytest.mark.parametrize("depth", [8, 4, 1])
@pytest.mark.parametrize("kernel,full,skip", KERNELS)
def test_red_skip_issues_half_the_stores(code_objects, kernel, full, skip, depth):
    functions, _ = code_objects
    n_full = _stores(functions[_one(functions, r"%d%s%s" % (len(kernel), kernel, re.escape(full % depth)))])
    n_skip = _stores(functions[_one(functions, r"%d%s%s" % (len(kernel), kernel, re.escape(skip % depth)))])
    assert n_full > 0 and n_full % 2 == 0, (kernel, depth, n_full)
    assert n_skip * 2 == n_full, (kernel, depth, n_full, n_skip)


@pytest.mark.parametrize("depth", list(range(1, 9)))
@pytest.mark.parametrize("kernel,full,skip", KERNELS)
def test_red_skip_register_budget(code_objects, kernel, full, skip, depth):
    _, notes = code_objects
    name = _one(notes, r"%d%s%s" % (len(kernel), kernel, re.escape(skip % depth)))
    n = notes[name]
    assert n.get("vgpr_count", 0) <= 256, (name, n)
    assert n.get("vgpr_spill_count", 0) == 0 and n.get("sgpr_spill_count", 0) == 0, (name, n)


@pytest.mark.parametrize("depth", [8, 4, 1])
def test_multi_keeps_its_budget(code_objects, depth):
    # k_fused_multi now holds both forms of the ordinary tile: still no vector spills (its few scalar spills, outside
    # the march, predate the flag)
    _, notes = code_objects
    for masked in (0, 1):
        name = _one(notes, r"13k_fused_multiILi%dELi2ELb%dEEEv" % (depth, masked))
        n = notes[name]
        assert n.get("vgpr_count", 0) <= 256, (name, n)
        assert n.get("vgpr_spill_count", 0) == 0, (name, n)
