"""GPU: the committed runs of the multigrid soak (tools/mg_soak.py on the cases of tests/mg_soak_cases.py) -- every served
mode of the multigrid PCG family on random shapes at the tile, tail and lane-count edges, against the numpy models and a
direct solve; see the tool for the checks A..E.  One test per (seed, chunk of 8 cases), and one for the cases that ever
failed (mg_soak_cases.REGRESSIONS)."""
import os
import sys

import pytest

import mg_soak_cases as sc

pytestmark = pytest.mark.gpu

CHUNK = 8
CHUNKS = [(seed, k) for seed, n in sc.COMMITTED for k in range((n + CHUNK - 1) // CHUNK)]


def soak():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import mg_soak
    return mg_soak


@pytest.mark.parametrize("seed,k", CHUNKS)
def test_committed_chunk(seed, k):
    n = dict(sc.COMMITTED)[seed]
    assert soak().run(sc.cases(seed, n)[k * CHUNK:(k + 1) * CHUNK]) == []


def test_regressions():
    """The cases that ever failed: the six of the first long run (NOTES R35.1), where the device was 17..94 x the model's
    distance from the direct solve because the model's sums, added in numpy's order, met the epsilon one iteration
    later.  mg_soak_cases.pcg_device_order now adds up in the device's order and takes the device's iterations."""
    assert soak().run([sc.case_from_repr(line) for line in sc.REGRESSIONS]) == []
