"""CPU: which kernels of the BUILT libccp_gs.so live in more than one gfx950 code object, and in how many.  A kernel
header that two sources include is compiled twice: build time and library size for nothing, and two copies to keep in
step.  The only kernels with several homes are the static ones of csrc/ccp_cg.hpp (the conjugate-gradient passes the CSR
path, the grid path, the multigrid PCG and the weighted handles' per-channel mode each instantiate) and of
csrc/ccp_grid_mg.hpp / ccp_grid_mgb.hpp (ccp_grid_mg.hip and ccp_grid_weighted.hip).  Splitting a source must not add
to this list; shortening it is welcome (then shorten HOMES).  Reads the code objects' resource notes only."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "coursecomputationalphotography_amd", "lib", "libccp_gs.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# kernel -> code objects that hold it, for every kernel held by more than one
HOMES = {
    "_ZN3ccpL10k_cg_alphaEPKdiPNS_7CgStateE": 4,
    "_ZN3ccpL10k_mg_checkEPKdidPNS_7CgStateE": 2,
    "_ZN3ccpL10k_mgb_betaEPKdliPNS_7CgStateE": 2,
    "_ZN3ccpL10k_mgb_initEPKdPdS2_lS2_l": 2,
    "_ZN3ccpL10k_mgb_tailENS_7MgTailTIdEEPKdPdlldiPKNS_7CgStateE": 2,
    "_ZN3ccpL10k_pcg_betaEPKdS1_idPNS_7CgStateE": 4,
    "_ZN3ccpL10k_pcg_initEPKdS1_PdlS2_": 4,
    "_ZN3ccpL11k_cg_updateEPdPKdS0_S2_lS0_PKNS_7CgStateE": 4,
    "_ZN3ccpL11k_mgb_alphaEPKdliPNS_7CgStateE": 2,
    "_ZN3ccpL11k_mgb_checkEPKdlidPNS_7CgStateE": 2,
    "_ZN3ccpL12k_mgb_updateEPdPKdS0_S2_lS0_lPKNS_7CgStateE": 2,
    "_ZN3ccpL12k_pcg_updateEPdPKdS0_S2_S2_lS0_S0_PKNS_7CgStateE": 4,
    "_ZN3ccpL13k_cg_residualEPdPKdlS0_PKNS_7CgStateE": 4,
    "_ZN3ccpL13k_cg_set_rlenEPKdiPNS_7CgStateE": 4,
    "_ZN3ccpL14k_cg_directionEPdPKdlPKNS_7CgStateE": 4,
    "_ZN3ccpL14k_mgb_set_rlenEPKdliPNS_7CgStateE": 2,
    "_ZN3ccpL15k_cg_axpy_finalEPdPKdS2_lPKNS_7CgStateE": 4,
    "_ZN3ccpL15k_mgb_directionEPdPKdlPKNS_7CgStateE": 2,
    "_ZN3ccpL15k_pcg_directionEPdPKdS2_lPKNS_7CgStateE": 4,
    "_ZN3ccpL15k_reduce_to_oneEPKdlPd": 4,
    "_ZN3ccpL16k_cg_alpha_fusedEPKdiiPNS_7CgStateE": 4,
    "_ZN3ccpL8k_cg_dotEPKdS1_lPdPKNS_7CgStateE": 4,
    "_ZN3ccpL9k_cg_betaEPKdidPNS_7CgStateE": 4,
    "_ZN3ccpL9k_cg_initEPKdPdS2_lS2_": 4,
    "_ZN3ccpL9k_mg_betaEPKdiPNS_7CgStateE": 2,
    "_ZN3ccpL9k_mg_tailENS_7MgTailTIdEEPKdPddiPKNS_7CgStateE": 2,
    "_ZN3ccpL9k_mgb_dotEPKdS1_lPdlPKNS_7CgStateE": 2,
}


def test_no_kernel_has_a_home_it_did_not_have(tmp_path):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libccp_gs.so or llvm-readelf missing")
    so = shutil.copy(LIB, tmp_path)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp_path)
    objs = sorted(str(p) for p in tmp_path.iterdir() if "gfx950" in p.name)
    assert objs, "no gfx950 code object in libccp_gs.so"
    homes = collections.Counter()
    for o in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        homes.update(set(re.findall(r"^\s+\.name:\s+(\S+)\s*$", notes, re.M)))
    assert len(homes) > 100, "the resource notes name hardly any kernel: the extraction is broken"
    assert {k: n for k, n in homes.items() if n > 1} == HOMES
