"""CPU: the segment planner of the wide red-black pass (csrc/ccp_wide_plan.hpp), through the host-only g++ driver
tests/cpp/wide_plan_check.cpp.

1. Over a sweep of rows, strips, channels, wave slots and depths the planned segments partition the interior rows
   exactly, every boundary lies an even number of rows from the first, no segment but an only one is shorter than
   the minimum height, and no other segment count is cheaper by the planner's own cost (ties: fewer segments).
2. Without border tiles the headline shape (16320 interior rows, 73 wide strips, 1 channel, 1024 wave slots, depth 8)
   gets 14 segments and 1022 tiles: one round.  BASELINE configs[1] (4032 rows, 18 strips x 3 channels) gets 18
   segments of 224 rows.
2b. With the border tiles those passes have (their march steps, their longest wave), the plan leaves the border kernel
   CUs of its own: 12 segments on both shapes, the counts that measured fastest (NOTES R12.1).
3. A plan of the chunk height (CCP_GS_WIDE_SEGMENTS=0) is the narrow tiling's interior chunks, row for row.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wide_plan") / "wide_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "wide_plan_check.cpp")])
    return exe


def plan(driver, rows, tiles_per_segment, slots, T, border=()):
    out = subprocess.run([driver, "plan", str(rows), str(tiles_per_segment), str(slots), str(T), *map(str, border)], check=True,
                         capture_output=True, text=True).stdout.split()
    n_seg, h, tiles, rounds, march = (int(v) for v in out)
    return {"n_seg": n_seg, "h": h, "tiles": tiles, "rounds": rounds, "march": march}


def test_sweep_partitions_and_minimum(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 10000


def test_headline_is_one_round_of_14_segments(driver):
    p = plan(driver, 16320, 73, 1024, 8)
    assert p == {"n_seg": 14, "h": 1166, "tiles": 1022, "rounds": 1, "march": 1200}


def test_config1_is_one_round_of_18_segments(driver):
    p = plan(driver, 4032, 18 * 3, 1024, 8)
    assert p == {"n_seg": 18, "h": 224, "tiles": 972, "rounds": 1, "march": 260}


def test_border_tiles_get_cus_of_their_own(driver):
    # 16384^2, R = 364: 338 top/bottom waves of 64 steps, 47 chunks x 2 side strips x 3 sub-tiles of 126 + 32 steps
    p = plan(driver, 16320, 73, 1024, 8, (338 * 64 + 47 * 2 * 3 * 158, 158))
    assert p == {"n_seg": 12, "h": 1360, "tiles": 876, "rounds": 1, "march": 1400}     # 219 CUs, 37 left free
    # 4096^2 x 3, R = 140: 82 top/bottom waves, 31 chunks x 2 x 4 sub-tiles of 36 + 32 steps, per channel
    p = plan(driver, 4032, 18 * 3, 1024, 8, (3 * (82 * 64 + 31 * 2 * 4 * 68), 68))
    assert p == {"n_seg": 12, "h": 336, "tiles": 648, "rounds": 1, "march": 380}       # 162 CUs, 94 left free
    # next to no border work still needs a CU: 14 segments leave none (256 blocks), 13 leave 18
    assert plan(driver, 16320, 73, 1024, 8, (100, 50))["n_seg"] == 13


def test_other_devices_and_small_grids(driver):
    # 304 CUs: 1216 slots hold 16 x 73 = 1168 tiles
    assert plan(driver, 16320, 73, 1216, 8)["n_seg"] == 16
    # fewer rows than two minimum segments: one segment
    assert plan(driver, 100, 3, 1024, 8) == {"n_seg": 1, "h": 100, "tiles": 3, "rounds": 1, "march": 140}
    # more tiles per segment than slots: rounds cannot be avoided, the planner still returns a partition
    p = plan(driver, 4096, 3000, 1024, 8)
    assert p["n_seg"] >= 1 and p["rounds"] == -(-p["tiles"] // 1024)
