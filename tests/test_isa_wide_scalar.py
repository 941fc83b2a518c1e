"""CPU: the scalar work in the march loop of the wide depth-8 kernels (ccp_grid_fused_wide.hpp), counted on the gfx950
ISA inside libccp_gs.so like tests/test_isa_wide.py.

A wide wave runs alone on its SIMD (its LDS ring holds the occupancy at one), so nothing overlaps the issue of its
scalar instructions.  The march addresses the rows of a ring turn through one buffer descriptor per plane and turn
(ccp_wide_plan.hpp, wide_turn_rows) instead of one per row.  The loop body is one turn: from the target of the
kernel's single backward branch to that branch.

1. Scalar instructions other than s_waitcnt and s_nop: at most 10 per stored row (it was 33 with a descriptor per row).
   The bound: three descriptors at an add / add-with-carry pair each would be 6, the rebuild of the three descriptors
   once per turn spread over its 20 steps about 2, loop control under 1.
2. No s_and_saveexec_b64 in the body: the compiler knows every descriptor to be wave-uniform, no waterfall loop.
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
RING = 20                     # kWideRing: march steps per turn
MAX_SCALAR_PER_ROW = 10


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> [(address, mnemonic, operands)] of both wide kernels"""
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("libccp_gs.so or llvm-objdump missing")
    d = tmp_path_factory.mktemp("isa_wide_scalar")
    so = shutil.copy(LIB, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    objs = sorted(str(p) for p in d.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    out = {}
    for o in objs:
        for name in WIDE.values():
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + name, o],
                                  check=True, capture_output=True, text=True).stdout
            body = []
            for line in text.splitlines():
                m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
                if m:
                    body.append((int(m.group(3), 16), m.group(1), m.group(2)))
            if body:
                out[name] = body
    assert set(out) == set(WIDE.values())
    return out


def loop_body(body):
    """the instructions from the target of the single backward branch up to that branch"""
    back = []
    for k, (addr, op, args) in enumerate(body):
        if op.startswith("s_cbranch") or op == "s_branch":
            # the simm16 is a signed count of dwords from the next instruction
            nxt = body[k + 1][0] if k + 1 < len(body) else addr + 4
            off = int(args.split()[0])
            off = off - 65536 if off >= 32768 else off
            target = nxt + 4 * off
            if target <= addr:
                back.append((target, addr))
    assert len(back) == 1, back
    lo, hi = back[0]
    return [(a, op, args) for a, op, args in body if lo <= a <= hi]


def is_scalar_work(op):
    return op.startswith("s_") and op not in ("s_waitcnt", "s_nop")


@pytest.mark.parametrize("store_red", [True, False])
def test_scalar_instructions_per_row(kernels, store_red):
    loop = loop_body(kernels[WIDE[store_red]])
    stores = sum(1 for _, op, _ in loop if op == "buffer_store_dwordx4")
    rows = stores // (2 if store_red else 1)
    assert rows == RING, (stores, rows)                      # the loop is one whole turn
    scalar = sum(1 for _, op, _ in loop if is_scalar_work(op))
    print(f"store_red={store_red}: {scalar} scalar instructions in {rows} steps, {scalar / rows:.2f} per row")
    assert scalar <= MAX_SCALAR_PER_ROW * rows, (scalar, rows)


@pytest.mark.parametrize("store_red", [True, False])
def test_no_waterfall_loops(kernels, store_red):
    loop = loop_body(kernels[WIDE[store_red]])
    assert sum(1 for _, op, _ in loop if op.startswith("s_and_saveexec")) == 0
