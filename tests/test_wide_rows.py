"""CPU: how a tile of the wide red-black pass addresses its rows (csrc/ccp_wide_plan.hpp: wide_march, wide_turn_rows,
wide_row_offset, wide_rows_stride_ok), through the host-only g++ driver tests/cpp/wide_rows_check.cpp.

The kernel (ccp_grid_fused_wide.hpp) builds one buffer descriptor per plane and ring turn from these functions and
leaves it to the range check which rows are read and written.  Exhaustive over local_rows 1..120, every ra < rb, both
parities of the block's first image row and every turn of the march:

1. the loads reach exactly the rows [m0, m1) and the stores exactly [ra, rb), each once, each at its own address;
2. every other row of a window gets an offset at or beyond num_records, or num_records is 0;
3. no offset wraps, every performed one is below 2^31, a lane that is out (2^31) stays out in every row;
4. no turn loads a row before m0 (the kernel skips rows only in the store window);
5. the stride guard trips where the offsets of kWideRing + 4 rows would pass 2^30, well before they reach 2^31.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wide_rows") / "wide_rows_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "wide_rows_check.cpp")])
    return exe


def test_sweep_selects_exactly_the_rows(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 500000


def test_usage(driver):
    assert subprocess.run([driver], capture_output=True).returncode == 2
