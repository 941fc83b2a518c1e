"""CPU: the line-smoother kernel's own source (csrc/ccp_grid_mgl.hpp) run on the host by a stand-alone program
(tests/cpp/mgl_host_check.cpp: a workgroup as 256 threads and a barrier) under AddressSanitizer and
UndefinedBehaviorSanitizer, against a serial long double Thomas solve: bounds of every global and LDS index, the
barriers, dead cells, both directions and parities, chunk remainders and single-cell lines.  No device is touched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path)
    shutil.copy(os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc", "ccp_grid_mgl.hpp"), d)
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "mgl_host", "ccp_grid_mg.hpp"), d)
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "mgl_host_check.cpp"), d)
    # the real kBlock, MgLevel and mg_at, as text: the stand-in header restates none of them
    csrc = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")
    common, mg = open(os.path.join(csrc, "ccp_common.hpp")).read(), open(os.path.join(csrc, "ccp_grid_mg.hpp")).read()
    parts = [re.search(r"^constexpr int kBlock = \d+;", common, re.M),
             re.search(r"^struct MgLevel \{.*?^\};", mg, re.M | re.S),
             re.search(r"^__host__ __device__ __forceinline__ long mg_at\(.*?^\}", mg, re.M | re.S)]
    assert all(parts), [bool(m) for m in parts]
    with open(os.path.join(d, "mgl_host_real.inc"), "w") as fh:
        fh.write("\n".join(m.group(0) for m in parts) + "\n")
    exe = os.path.join(d, "mgl_host_check")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I", d, os.path.join(d, "mgl_host_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "worst" in p.stdout
