"""CPU: the backward pass's kernel bodies (csrc/ccp_grid_adjoint.hpp: adjoint_pixel, adjoint_begin_pixel) run on the host
by a stand-alone program (tests/cpp/adjoint_host_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer.  Every
buffer is exactly its view's size, so no index may leave its view; the shapes are those of tests/test_gpu_adjoint.py, the
one-pixel-wide and one-pixel-tall ones included, and the values are compared exactly with a plain raster-order
restatement.  No device is touched and nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_kernel_bodies_on_the_host_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path)
    csrc = os.path.join(ROOT, "coursecomputationalphotography_amd", "csrc")
    shutil.copy(os.path.join(csrc, "ccp_grid_adjoint.hpp"), d)
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "adjoint_host_check.cpp"), d)
    # the real kBlock and w_at, as text: the host build restates neither
    common, weighted = open(os.path.join(csrc, "ccp_common.hpp")).read(), open(os.path.join(csrc, "ccp_grid_stencil.hpp")).read()
    parts = [re.search(r"^constexpr int kBlock = \d+;", common, re.M),
             re.search(r"^__host__ __device__ __forceinline__ long w_at\(.*?^\}", weighted, re.M | re.S)]
    assert all(parts), [bool(m) for m in parts]
    with open(os.path.join(d, "adjoint_host_real.inc"), "w") as fh:
        fh.write("namespace ccp {\n" + "\n".join(m.group(0) for m in parts).replace("__host__ __device__ __forceinline__", "inline")
                 + "\n}\n")
    exe = os.path.join(d, "adjoint_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-I", d, os.path.join(d, "adjoint_host_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert re.search(r"checked \d{6,} values, 0 mismatches", p.stdout)
