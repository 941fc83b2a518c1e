"""GPU: the five multigrid options of a grid handle (include/ccp_gs.h: ccp_grid_mg_set_ / _get_ hierarchy, precision,
channels, smoother, nullspace) through the C ABI, one table for all five: which values a setter takes, when it returns
CCP_ERR_UNSUPPORTED, and what a change of value does to what ccp_grid_mg_prepare built.

| option    | values | UNSUPPORTED when           | a change of value                                              |
| hierarchy | 0, 1   | the handle is not weighted | drops what prepare built; set back, it stays dropped           |
| precision | 0, 1   | F32 on a row block         | the same                                                       |
| channels  | 0, 1   | never                      | the same                                                       |
| smoother  | 0, 1   | never                      | the same                                                       |
| nullspace | 0, 1   | the handle is not weighted | refuses the enqueue call while it lasts; set back, it runs again |

A setter checks in this order: the handle (NULL: BAD_ARG), the value's range (BAD_ARG), UNSUPPORTED (even for the value
the handle holds), the same value (CCP_OK, nothing happens).  Handles: weighted 33x17 C = 2 (one level above the tail),
structured 33x17, a row block of 33x17 (9 rows, ghost 1, no communicator).  The solves are enqueue solves of 5
iterations; equality is of bits, to a twin handle that no setter touched after its prepare."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_mg_enqueue as tge
from coursecomputationalphotography_amd import capi

pytestmark = pytest.mark.gpu

OK, BAD_ARG, STATE, UNSUPPORTED = 0, 1, 5, 6
W, H, CN = 33, 17, 2
CAP, SEED = 5, 41
OPTIONS = ("hierarchy", "precision", "channels", "smoother", "nullspace")
WEIGHTED_ONLY = ("hierarchy", "nullspace")
# the prepared configuration: rescaled, fp64, sequential, point, none
PREPARED = {"hierarchy": 1, "precision": 0, "channels": 0, "smoother": 0, "nullspace": 0}


def setter(g, option, value):
    return getattr(g.L, f"ccp_grid_mg_set_{option}")(g.h, value)


def getter(g, option):
    value = C.c_int32(-9)
    assert getattr(g.L, f"ccp_grid_mg_get_{option}")(g.h, C.byref(value)) == OK
    return value.value


def weighted():
    g = capi.Grid(W, H, CN, weighted=True)
    g.set_weights(*tge.screened(W, H, 31 * W + H))
    return g


@pytest.mark.parametrize("option", OPTIONS)
def test_statuses(option):
    lib = capi.load()
    value = C.c_int32(-9)
    for v in (-1, 0, 1, 2):
        assert getattr(lib, f"ccp_grid_mg_set_{option}")(None, v) == BAD_ARG
    assert getattr(lib, f"ccp_grid_mg_get_{option}")(None, C.byref(value)) == BAD_ARG and value.value == -9
    handles = {"weighted": weighted(), "structured": capi.Grid(W, H, 1),
               "row block": capi.Grid(W, H, 1, row_begin=0, row_count=9, ghost=1)}
    for name, g in handles.items():
        assert getattr(g.L, f"ccp_grid_mg_get_{option}")(g.h, None) == BAD_ARG
        assert getter(g, option) == 0, name                   # every default is 0
        served = [0, 1]
        if option in WEIGHTED_ONLY and name != "weighted":
            served = []                                       # ... not even the value the handle holds
        elif option == "precision" and name == "row block":
            served = [0]
        held = 0
        for v in (1, -1, 2, 1, 0, 2, -1, 0, 1):
            want = BAD_ARG if v in (-1, 2) else OK if v in served else UNSUPPORTED
            assert setter(g, option, v) == want, (name, v)
            if want == OK:
                held = v
            assert getter(g, option) == held, (name, v)       # a refused set leaves the value as it was
        for other in OPTIONS:                                 # and no setter writes another option's value
            if other != option:
                assert getter(g, other) == 0, (name, other)
        g.close()


def prepared():
    g = weighted()
    for option in OPTIONS:
        assert setter(g, option, PREPARED[option]) == OK
    tge.load(g, SEED)
    g.mg_prepare(0)
    return g


def solve(g):
    """An enqueue solve from the start vector of tge.load: (the bits of every channel's x, the bits of the report)"""
    g.randomize_x(SEED + 1, 0.0, 255.0)
    report = torch.full((g.C, 6), tge.SENTINEL, dtype=torch.float64, device=tge.DEV)
    g.mg_conjugate_gradient_enqueue(0.0, CAP, 0, report)
    torch.cuda.synchronize()
    rep = report.cpu().numpy()
    assert (rep[:, 0] == CAP).all(), rep
    return [tge.bits(g.get_x(c)).copy() for c in range(g.C)], tge.bits(rep).copy()


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got[0], want[0])) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("option", OPTIONS)
def test_what_a_setter_does_to_a_prepared_handle(option):
    twin, g = prepared(), prepared()
    want = solve(twin)
    assert setter(g, option, PREPARED[option]) == OK          # the same value: nothing happens
    assert same(solve(g), want)
    g.randomize_x(SEED + 1, 0.0, 255.0)
    assert setter(g, option, 1 - PREPARED[option]) == OK      # a changed value
    assert getter(g, option) == 1 - PREPARED[option]
    tge.refused(g, STATE, cap=CAP)
    assert setter(g, option, PREPARED[option]) == OK          # set back
    if option == "nullspace":                                 # nothing was freed: the prepared configuration is back
        assert same(solve(g), want)
    else:
        tge.refused(g, STATE, cap=CAP)                        # what the change freed stays freed
        g.mg_prepare(0)
        assert same(solve(g), want)
    assert same(solve(twin), want)                            # (the twin still gives the same bits)
    twin.close(), g.close()
