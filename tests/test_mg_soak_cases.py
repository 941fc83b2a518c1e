"""CPU: the case generator of the multigrid soak (tests/mg_soak_cases.py) -- determinism, what the committed runs cover,
and that every committed system is one the numpy model of its mode solves: the GPU test (tests/test_gpu_mg_soak.py)
must not hide a failure behind a system no solver could solve."""
import collections

import numpy as np
import pytest

import mg_soak_cases as sc
import mode_walk_helpers as mw
import neumann_helpers as nh

CHUNK = 8
ALL = sc.committed_cases()
CHUNKS = [(seed, k) for seed, n in sc.COMMITTED for k in range((n + CHUNK - 1) // CHUNK)]


def deltas(case):
    return {s - m for s in (case.W, case.H) for m in sc.TILE_SIDES if s - m in sc.DELTAS}


def test_cases_are_deterministic_and_repr_round_trips():
    for seed, n in sc.COMMITTED:
        a, b = sc.cases(seed, n), sc.cases(seed, n)
        assert a == b and len(a) == n
        assert sc.cases(seed, 5) == sc.cases(seed, 5)
        for case in a:
            line = repr(case)
            assert "\n" not in line
            again = sc.case_from_repr(line)
            assert again == case and repr(again) == line
    assert sc.cases(1, 64) != sc.cases(2, 64)
    assert all(sc.case_from_repr(line) for line in sc.REGRESSIONS)
    with pytest.raises(ValueError):
        sc.case_from_repr("print(1)")


def test_committed_runs_cover_every_mode_class_and_edge():
    modes = collections.Counter(sc.mode_of(c) for c in ALL)
    for kind in mw.KINDS:
        for m in mw.served_modes(kind):
            assert modes[(kind,) + m] >= 2, (kind, m)
    assert sum(c.nullspace == "constant" for c in ALL) >= 3
    for smoother in ("point", "line"):
        assert {c.nu for c in ALL if c.smoother == smoother} == {1, 2, 3, 4}, smoother
    ops = collections.Counter(c.op for c in ALL)
    for name in sc.OPERATOR_CLASSES + sc.MASK_CLASSES:
        assert ops[name] >= 2, name
    assert set(sc.B) <= {c.W for c in ALL} and set(sc.B) <= {c.H for c in ALL}
    assert len(sc.B) == 28 and set(sc.B) == {1, 2, 3, 4} | {m + d for m in (16, 32, 64, 96, 128, 192) for d in (-1, 0, 1, 2)}
    for name, has in (("f32", lambda c: c.precision == "f32"), ("batched", lambda c: c.channels == "batched"),
                      ("line", lambda c: c.smoother == "line")):
        assert set().union(*(deltas(c) for c in ALL if has(c))) == set(sc.DELTAS), name
    for side in sc.LONG_SIDES:
        assert any(c.W == side and c.H < side for c in ALL) and any(c.H == side and c.W < side for c in ALL), side
    assert sum(sc.is_long_thin(c) for c in ALL) * 8 == len(ALL)


def test_every_emitted_configuration_is_served():
    for seed in (1, 2, 7, 11):
        for case in sc.cases(seed, 256):
            op = "S" if case.kind == "structured" else "M" if case.kind == "mask" else "A"
            assert not mw.reasons(case.kind, (case.precision, case.channels, case.smoother, case.hierarchy, op)), case
            assert case.W * case.H <= sc.AREA and 1 <= case.C <= 3 and 1 <= case.nu <= 4, case
            assert case.scales[0] == max(case.scales) and len(case.scales) == case.C, case
            if case.kind != "weighted":
                assert (case.hierarchy, case.nullspace) == ("galerkin", "none"), case
            if case.nullspace == "constant":
                assert case.op == "floating" and case.channels == "sequential" and min(case.W, case.H) >= 2, case
                assert case.smoother == "point" or nh.line_served(case.W, case.H), case
            else:
                assert case.op != "floating", case


@pytest.mark.parametrize("seed,k", CHUNKS)
def test_the_models_solve_every_committed_case(seed, k):
    n = dict(sc.COMMITTED)[seed]
    for case in sc.cases(seed, n)[k * CHUNK:(k + 1) * CHUNK]:
        built = sc.build(case)
        for c in range(case.C):
            assert float(np.linalg.norm(built.b[c])) > 0.0, (case, c)
            x, its, converged, norm = sc.model_pcg(built, c, 60)
            assert converged and its <= 60, (case, c, its, norm, built.eps)
            ref, solved = sc.direct(built, c)
            dist = sc.distance(built, c, x, ref, solved)
            assert np.isfinite(dist), (case, c)
            _, z, dev = sc.model_vcycle(built, c)
            assert np.all(np.isfinite(z)), (case, c)
            if case.smoother == "line":
                assert dev is not None and np.isfinite(dev), (case, c, dev)
            print(f"{case.op} {case.W}x{case.H} channel {c}: {its} iterations, |x - direct| {dist:.3e}, line deviation {dev}")
