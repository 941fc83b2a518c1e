"""CPU: the planner of the temporally blocked red-black pass (csrc/ccp_fused_plan.hpp), through the host-only g++ driver
tests/cpp/fused_plan_check.cpp.

(a) Over the shapes of (c), every depth 1..8 and the pass kinds (unchecked, checked, edge hand-off, masked, one of several
    passes in a launch, the debug and A/B switches) the driver checks the plan's invariants: chunks partition the stored
    rows, the dispatch order is a bijection with the edge chunks first, every (chunk, strip) tile runs in exactly one of the
    two launches with side sub-tiles that partition their chunk, the wide tiles cover exactly what the ordinary narrow
    tiles would store, the hand-off's wave count is the number of edge-chunk waves, the stored rows never reach past the
    owned rows and lose 2T per pass on a stale side only; and the split of an iteration count into passes sums up, is
    even unless an odd one was allowed and is cheaper, and is sorted by depth.
(b) The figures the project records for the two benchmark shapes at depth 8 on 256 CUs (NOTES 4.1, R12.1).
(c) The restatements the GPU tests use — rowblock_sweep_helpers.block_interior, depth8_passes and wide_strips,
    test_gpu_wide_segments.interior_rows — agree with the planner on the shapes of those tests and on a grid of small ones.
"""
import itertools
import os
import shutil
import subprocess

import pytest

from rowblock_sweep_helpers import CASES, block_interior, depth8_passes, first_local_rows, wide_strips
from test_gpu_wide_segments import SHAPES, interior_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

WS = [1, 2, 95, 96, 97, 224, 225, 300, 641]
HS = [1, 2, 63, 64, 65, 80, 81, 129, 400]
RS = [16, 32, 48, 50, 140]
GHOSTS = [2, 16, 32]
CUS = 256


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fused_plan") / "fused_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fused_plan_check.cpp")])
    return exe


def block(H, cuts, ghost, i):
    """(y0, local rows, own_lo, own_hi, ghost_top, ghost_bottom) of block i, as ccp_grid_create lays it out"""
    top, bottom = min(ghost, cuts[i]), min(ghost, H - cuts[i + 1])
    return cuts[i] - top, top + cuts[i + 1] - cuts[i] + bottom, top, top + cuts[i + 1] - cuts[i], top, bottom


def case(W, H, C, R, T, blk=None, ghost=0, since=0, k=0, l1=0, edge_rows=0, masked=0, multi=0, short_edges=1, all_border=0,
         side_rows=0, wide=1, wide_segments=-1, send=(0, 0)):
    y0, local, own_lo, own_hi, top, bottom = blk or (0, H, 0, H, 0, 0)
    return (W, H, C, y0, local, own_lo, own_hi, ghost, top, bottom, send[0], send[1], R, T, CUS, since, k, l1, edge_rows, masked,
            multi, short_edges, all_border, side_rows, wide, wide_segments)


def run_batch(driver, cases, parse=True):
    """per case the plan's fields (parse=False: the line), None where the pass does not run (ghosts exhausted, nothing to store)"""
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([driver, "batch"], input=text, capture_output=True, text=True)
    fails = [ln for ln in out.stdout.splitlines() if ln.startswith("FAIL")]
    assert out.returncode == 0 and not fails, "\n".join(fails[:20]) or out.stdout[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    if not parse:
        return [None if ln == "skip" else ln for ln in lines]
    return [None if ln == "skip" else {k: int(v) for k, v in (f.split("=") for f in ln.split())} for ln in lines]


def odd_cuts(H, ghost):
    """row blocks of an H-row image of which one at least starts on an odd local row 0"""
    if H < 6:
        return None
    cuts = [0, H // 3 | 1, 2 * H // 3, H]
    for a in (0, 1):
        cuts[2] = 2 * H // 3 + a
        if cuts[1] < cuts[2] < H and any(y & 1 for y in first_local_rows(cuts, ghost)):
            return cuts
    return None


def small_grid(Ts=range(1, 9)):
    """whole images and row blocks of the small shapes: [(case, what it is)]"""
    out = []
    for W, H, R, T in itertools.product(WS, HS, RS, Ts):
        out.append((case(W, H, 1 + (W + H) % 3, R, T), ("whole", W, H, R, T)))
        for ghost in GHOSTS:
            cuts = odd_cuts(H, ghost)
            if cuts is None:
                continue
            for i in range(len(cuts) - 1):
                for k in range(min(3, max(1, ghost // (2 * T)))):
                    out.append((case(W, H, 1 + (W + H) % 3, R, T, block(H, cuts, ghost, i), ghost, k=k),
                                ("block", W, H, R, T, cuts, ghost, i, k)))
    return out


def test_header_compiles_alone():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + CSRC, "-x", "c++", "-"],
                   input='#include "ccp_fused_plan.hpp"\nint main() { return ccp::fused_plan(ccp::FusedPlanInput(), ccp::FusedPassKind()).T; }\n',
                   text=True, check=True)


def test_invariants_over_kinds(driver):
    """(a) on the small grid and the GPU tests' shapes, for every kind of pass"""
    cases = []
    kinds = [dict(), dict(l1=1), dict(l1=2), dict(masked=1), dict(multi=1), dict(masked=1, multi=1), dict(short_edges=0),
             dict(all_border=1), dict(side_rows=6), dict(wide=0), dict(wide_segments=0), dict(wide_segments=3)]
    for c, what in small_grid():
        W, H, R, T = what[1:5]
        if what[0] == "whole":
            cases += [case(W, H, c[2], R, T, **kw) for kw in kinds if T == 8 or not any(k.startswith("wide") for k in kw)]
        else:
            cuts, ghost, i, k = what[5:]
            blk = block(H, cuts, ghost, i)
            cases.append(c)
            # the pass whose result is exchanged: the neighbours' rows first, as many as they take
            edge_rows, send = ((16, (0, 0)), (2 * T, (7, 40)), (ghost, (0, 0)))[(i + k) % 3]
            cases.append(case(W, H, c[2], R, T, blk, ghost, k=k, edge_rows=edge_rows, send=send))
            if k == 0:
                cases.append(case(W, H, c[2], R, T, blk, ghost, since=3, multi=1))
    for name, (W, H, C, cuts, ghost, R, _, _) in CASES.items():
        for i in range(len(cuts) - 1):
            for k in range(ghost // 16):
                for kw in (dict(), dict(edge_rows=16), dict(edge_rows=ghost), dict(wide_segments=0), dict(wide_segments=3), dict(l1=1)):
                    cases.append(case(W, H, C, R, 8, block(H, cuts, ghost, i), ghost, k=k, **kw))
    for W, H, C, R, _ in SHAPES + [(1123, 463, 2, 32, None)]:
        for T in range(1, 9):
            cases += [case(W, H, C, R, T, **kw) for kw in kinds if T == 8 or not any(k.startswith("wide") for k in kw)]
    plans = run_batch(driver, cases, parse=False)
    assert sum(p is not None for p in plans) > 20000
    assert sum(p is not None and " wide=1 " in p for p in plans) > 500 and sum(p is not None and " edge=1 " in p for p in plans) > 500


def test_pass_split_invariants(driver):
    out = subprocess.run([driver, "splits"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 8000


def split(driver, iterations, tmax, free, costs=()):
    out = subprocess.run([driver, "split", str(iterations), str(tmax), str(int(free)), *map(str, costs)], check=True, capture_output=True,
                         text=True).stdout.split()
    return int(out[0]), bool(int(out[1])), [int(v) for v in out[2:]]


def test_pass_splits_the_project_records(driver):
    # 50 iterations at depth <= 8 need seven passes; where x must come back in place it takes eight (ccp_grid.hip, allow_swap)
    in_place, free, depths = split(driver, 50, 8, False)
    assert (in_place, free, len(depths), sum(depths)) == (0, False, 8, 50)
    in_place, free, depths = split(driver, 50, 8, True)
    assert (in_place, free, len(depths), sum(depths)) == (0, True, 7, 50)
    # a count that an even number of deepest passes covers is split that way, allowed to swap or not
    assert split(driver, 32, 8, True) == (0, False, [8, 8, 8, 8])
    assert split(driver, 9, 8, False) == (0, False, [8, 1])
    # depth-1 passes only: the odd iteration goes through the in-place kernels
    assert split(driver, 7, 1, False) == (1, False, [1] * 6)
    assert split(driver, 6, 1, True) == (0, False, [1] * 6)
    # measured costs: a depth that is far cheaper per iteration carries the split
    assert split(driver, 12, 4, False, (1.0, 1.9, 0.3, 3.9)) == (0, False, [3, 3, 3, 3])


def test_tune_candidates_hold_the_benchmark_chunk_heights(driver):
    """ccp_grid_tune's rounds-1..4 heights at depth 8 with 2 waves per SIMD on 256 CUs: 364 rows fill four rounds at
    16384^2 (43 blocks across, 2 short chunks), 140 rows two rounds at 4096^2 x 3 (11 blocks x 3)"""
    fixed = [32, 48, 64, 80, 96, 112, 128, 160, 192, 256]
    out = subprocess.run([driver, "tune", "16384", "16384", "0", "16384", "1", "8", "512"], check=True, capture_output=True, text=True)
    assert [int(v) for v in out.stdout.split()] == fixed + [778, 496, 364]
    out = subprocess.run([driver, "tune", "4096", "4096", "0", "4096", "3", "8", "512"], check=True, capture_output=True, text=True)
    assert [int(v) for v in out.stdout.split()] == fixed + [312, 140, 92, 68]


def test_recorded_figures_of_the_benchmark_shapes(driver):
    """(b)"""
    big, mid = run_batch(driver, [case(16384, 16384, 1, 364, 8), case(4096, 4096, 3, 140, 8)])
    assert (big["n_chunks"], big["n_strips"], big["grid_x"]) == (47, 171, 43)
    assert big["edge_chunks"] * (big["n_strips"] - big["edge_strips"]) == 338 and big["first_rows"] + 32 == big["last_rows"] + 32 == 64
    assert (big["side_subs"], big["side_rows"]) == (3, 126)
    assert (big["border_steps"], big["border_longest"]) == (338 * 64 + 47 * 2 * 3 * 158, 158)
    assert (big["n_wide"], big["wide_y1"] - big["wide_y0"]) == (73, 16320)
    assert (big["wide_nseg"], big["wide_h"], big["wide_tiles"]) == (12, 1360, 876)
    assert (mid["n_chunks"], mid["n_strips"]) == (31, 43)
    assert mid["edge_chunks"] * (mid["n_strips"] - mid["edge_strips"]) == 82 and mid["first_rows"] + 32 == mid["last_rows"] + 32 == 64
    assert (mid["side_subs"], mid["side_rows"]) == (4, 36)
    assert (mid["border_steps"], mid["border_longest"]) == (3 * (82 * 64 + 31 * 2 * 4 * 68), 68)
    assert (mid["n_wide"], mid["wide_y1"] - mid["wide_y0"]) == (18, 4032)
    assert (mid["wide_nseg"], mid["wide_h"], mid["wide_tiles"]) == (12, 336, 648)


def check_interior(plan, want, what):
    """block_interior's answer against the plan of the same pass"""
    if want is None:
        assert plan["edge_chunks"] == plan["n_chunks"], what
        return
    assert (plan["nb_top"], plan["nb_bot"]) == want[:2] and plan["edge_chunks"] < plan["n_chunks"], what
    if plan["wide"]:
        assert (plan["wide_y0"], plan["wide_y1"]) == want[2:], what


def check_columns(plan, W, what):
    n = wide_strips(W)
    assert n == -(-(plan["wx1"] - plan["wx0"]) // 224), what
    if plan["any_plain"]:
        assert n == plan["n_wide"], what


def test_restatements_agree_on_the_gpu_tests_shapes(driver):
    """(c) CASES and the shapes of tests/test_gpu_wide_segments.py"""
    cases, wants = [], []
    for name, (W, H, C, cuts, ghost, R, _, _) in CASES.items():
        for i, passes in enumerate(depth8_passes(H, cuts, ghost, R, ghost // 16)):
            for k, want in enumerate(passes):
                cases.append(case(W, H, C, R, 8, block(H, cuts, ghost, i), ghost, k=k))
                wants.append((name, i, k, W, want))
    n_wide_passes = 0
    for plan, (name, i, k, W, (st_lo, st_hi, interior)) in zip(run_batch(driver, cases), wants):
        if plan is None:
            assert st_hi <= st_lo, (name, i, k)
            continue
        assert (plan["st_lo"], plan["st_hi"]) == (st_lo, st_hi), (name, i, k)
        check_interior(plan, interior, (name, i, k))
        check_columns(plan, W, (name, i, k))
        n_wide_passes += plan["wide"]
    assert n_wide_passes >= 20
    shapes = SHAPES + [(1123, 463, 2, 32, None)]
    for mode in (-1, 0, 3):
        plans = run_batch(driver, [case(W, H, C, R, 8, wide_segments=mode) for W, H, C, R, _ in shapes])
        for plan, (W, H, C, R, _) in zip(plans, shapes):
            assert plan["wide"] == 1, (W, H)
            assert (plan["wide_y0"], plan["wide_y1"]) == interior_rows(H, R), (W, H, R)
            check_columns(plan, W, (W, H))
            check_interior(plan, block_interior(H, 0, 0, H, R), (W, H, R))
            rows = plan["wide_y1"] - plan["wide_y0"]
            if mode == 0:
                assert (plan["wide_nseg"], plan["wide_h"]) == (-(-rows // R), R), (W, H, R)
            if mode == 3:
                h = -(-rows // 3) + (-(-rows // 3) & 1)
                assert (plan["wide_nseg"], plan["wide_h"]) == (-(-rows // h), h), (W, H, R)
            assert plan["wide_tiles"] == plan["wide_stride"] * plan["wide_nseg"] * C, (W, H, R)


def test_restatements_agree_on_the_small_grid(driver):
    """(c) the grid of small shapes, depth 8: whole images and row blocks with an odd first local row, ghosts 2, 16, 32"""
    grid = small_grid(Ts=[8])
    plans = run_batch(driver, [c for c, _ in grid])
    compared = odd_first = 0
    for plan, (c, what) in zip(plans, grid):
        W, H, R = what[1:4]
        if what[0] == "whole":
            assert plan is not None, what
            check_interior(plan, block_interior(H, 0, 0, H, R), what)
            check_columns(plan, W, what)
            if plan["edge_chunks"] < plan["n_chunks"]:
                y0, y1 = interior_rows(H, R)
                if plan["wide"]:
                    assert (plan["wide_y0"], plan["wide_y1"]) == (y0, y1), what
                    compared += 1
            else:
                with pytest.raises(AssertionError):
                    interior_rows(H, R)
        else:
            cuts, ghost, i, k = what[5:]
            passes = depth8_passes(H, cuts, ghost, R, k + 1)[i]
            st_lo, st_hi, interior = passes[k]
            if 2 * 8 * (k + 1) > ghost:                                  # the ghosts do not carry a depth-8 pass
                assert plan is None, what
                continue
            if plan is None:
                assert st_hi <= st_lo, what
                continue
            assert (plan["st_lo"], plan["st_hi"]) == (st_lo, st_hi), what
            check_interior(plan, interior, what)
            check_columns(plan, W, what)
            odd_first += c[3] & 1
    assert compared >= 20 and odd_first >= 100
