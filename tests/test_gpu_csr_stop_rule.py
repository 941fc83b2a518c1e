"""GPU: the stop rule of the three stored-matrix Gauss-Seidel drivers of ccp_csr_gauss_seidel (check_every >= 1) at the
positions where each can go wrong: the one-workgroup kernel (rule on the device), the pipelined level schedule (the host
looks at 128 sweeps at a time and re-runs from a snapshot) and the per-group loop (the device's `active` word, read back
every 8 checks) — in index and in colour order, and the per-group loop on a one-rank row block over real RCCL.

The system is the 17x13 Poisson matrix (221 rows; 29 levels of at most 13 rows in index order, so every driver accepts it),
kept on the stored matrix by CCP_GS_STRUCTURED=0.  Expectations come from the oracle alone (tests/stop_rule_helpers.py): one
sweep at a time, b and x0 scaled so that the steps cross epsilon at the wanted checked sweep, the stop read off the scaled
system's own steps, every checked step at least MARGIN away from epsilon."""
import numpy as np
import pytest

import oracle
import stop_rule_helpers as srh

pytestmark = pytest.mark.gpu

EPS = 0.5
W, H = 17, 13

# (check_every, max_iteration, stop sweep or None: the cap is reached)
POSITIONS = [
    (1, 140, 5),
    (1, 140, 128),      # last sweep of the pipeline's first batch of 128: no re-run
    (1, 140, 129),      # first sweep of the second batch
    (1, 130, None),     # a second batch of 2 sweeps
    (3, 140, 6),
    (3, 140, 129),
    (3, 13, None),      # the cap falls between checks
    (1, 8, 8),          # end of the per-group loop's batch of 8 checks
    (1, 9, 9),          # first check of the next batch of 8
    (1, 13, None),
    (1, 0, None),       # cap 0: 0 iterations, not converged, x still the bits of the start
]

# (order, environment): which driver sweeps
DRIVERS = {
    "index-one_workgroup": ("index", {}),
    "index-pipeline": ("index", {"CCP_GS_ONE_BLOCK": "0"}),
    "index-per_group": ("index", {"CCP_GS_ONE_BLOCK": "0", "CCP_GS_PIPELINE": "0"}),
    "colour-one_workgroup": ("colour", {}),
    "colour-per_group": ("colour", {"CCP_GS_ONE_BLOCK": "0"}),
}


@pytest.fixture(scope="module")
def capi():
    from coursecomputationalphotography_amd import capi
    assert capi.device_count() >= 1
    return capi


class IndexOrder(srh.System):
    """The same matrix swept in the order of its indices: the identity for the oracle's permutation."""

    def __init__(self, orc, w, h):
        super().__init__(orc, w, h)
        self.perm = np.arange(self.n, dtype=np.int32)
        self._m = orc.from_csr(self.v, self.c, self.r)


_systems, _channels = {}, {}


def channel(orc, order, every, cap, stop):
    """The scaled system of one position and what the oracle says of it, computed once."""
    if order not in _systems:
        _systems[order] = IndexOrder(orc, W, H) if order == "index" else srh.System(orc, W, H)
    key = (order, every, cap, stop)
    if key not in _channels:
        _channels[key] = srh.Channel(_systems[order], stop, every, EPS, cap, seed=100 * every + cap)
    return _systems[order], _channels[key]


def check(capi, m, order, c, every, cap, what):
    ordering = capi.ORDER_LEXICOGRAPHIC if order == "index" else capi.ORDER_MULTICOLOUR
    x, rep = m.gauss_seidel(c.b, EPS, cap, x0=c.x0, check_every=every, ordering=ordering)
    assert m.last_path() == "sliced ELL", what
    it, conv, last = c.stop
    print(what, "iterations", rep.iterations, it, "converged", rep.converged, conv, "last step", rep.last_l1_step, last)
    assert (rep.iterations, rep.converged) == (it, conv), (what, rep.iterations, rep.converged, c.stop)
    assert abs(rep.last_l1_step - last) <= 1e-9 * last, (what, rep.last_l1_step, last)
    assert np.array_equal(x, c.x), (what, np.abs(x - c.x).max())


@pytest.mark.parametrize("every,cap,stop", POSITIONS)
@pytest.mark.parametrize("driver", list(DRIVERS))
def test_stored_matrix_driver_stops_where_the_oracle_stops(capi, orc, monkeypatch, driver, every, cap, stop):
    order, env = DRIVERS[driver]
    monkeypatch.setenv("CCP_GS_STRUCTURED", "0")
    for k in ("CCP_GS_ONE_BLOCK", "CCP_GS_PIPELINE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, c = channel(orc, order, every, cap, stop)
    m = capi.CsrMatrix().upload_compressed(s.v, s.c, s.r)        # (the switches are read here)
    if order == "colour":
        m.set_colouring(oracle.grid_colour(W, H), 2)
    check(capi, m, order, c, every, cap, (driver, every, cap, stop))
    m.close()


@pytest.mark.parametrize("every,cap,stop", [(1, 140, 5), (3, 13, None), (1, 0, None)])
@pytest.mark.parametrize("overlap", ["as_set_up", "off"])
def test_one_rank_row_block_per_group_loop_stops_where_the_oracle_stops(capi, orc, monkeypatch, overlap, every, cap, stop):
    """ccp_csr_upload_rows at world 1 through the process's real RCCL: the per-group loop in colour order with the
    exchange hidden behind the inner slices (as the upload sets it up) and with CCP_GS_ROWS_OVERLAP=0."""
    try:
        capi.comm_probe(0)
    except capi.CcpError as e:
        pytest.skip(f"no communicator here: {e}")
    monkeypatch.setenv("CCP_GS_STRUCTURED", "0")
    monkeypatch.delenv("CCP_GS_ONE_BLOCK", raising=False)
    if overlap == "off":
        monkeypatch.setenv("CCP_GS_ROWS_OVERLAP", "0")
    else:
        monkeypatch.delenv("CCP_GS_ROWS_OVERLAP", raising=False)
    s, c = channel(orc, "colour", every, cap, stop)
    comm = capi.Comm(capi.comm_unique_id(), 0, 1, 0)
    m = capi.CsrMatrix().upload_rows(comm, 0, s.n, s.v, s.c, s.r[:-1], np.diff(s.r), oracle.grid_colour(W, H), 2)
    check(capi, m, "colour", c, every, cap, ("row block", overlap, every, cap, stop))
    m.close()
    comm.close()
