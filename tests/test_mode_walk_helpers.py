"""CPU: the model of the multigrid mode switches (tests/mode_walk_helpers.py) and the walks that
tests/test_gpu_mg_transitions.py runs on the device.  `expected_status` is checked against the header's lists of refused
combinations, case by case; the committed walks (WALKS: seed and length per handle kind, at most 64 steps) must contain
every step kind at least twice, every served mode directly after a change of the operator, and every refusal reason
alone in a configuration that a served solve follows.  A seed or a length that loses one of these fails here, on the
CPU."""
import pytest

import mode_walk_helpers as mw

OK, BAD_ARG, STATE, UNSUPPORTED = 0, 1, 5, 6


def config(precision="f64", channels="sequential", smoother="point", hierarchy="galerkin", op="A"):
    return (precision, channels, smoother, hierarchy, op)


def test_status_values_are_the_headers():
    assert (mw.OK, mw.BAD_ARG, mw.STATE, mw.UNSUPPORTED) == (OK, BAD_ARG, STATE, UNSUPPORTED)


def test_expected_status_follows_the_contract():
    for hierarchy in ("galerkin", "rescaled"):
        for op in ("A", "B", "Afixed", "Bfixed"):
            served = [config(hierarchy=hierarchy, op=op), config("f32", hierarchy=hierarchy, op=op),
                      config(channels="batched", hierarchy=hierarchy, op=op), config(smoother="line", hierarchy=hierarchy, op=op)]
            for c in served:
                assert mw.expected_status("weighted", c) == OK, c
            refused = [config("f32", "batched", hierarchy=hierarchy, op=op), config("f32", smoother="line", hierarchy=hierarchy, op=op),
                       config(channels="batched", smoother="line", hierarchy=hierarchy, op=op),
                       config("f32", "batched", "line", hierarchy=hierarchy, op=op)]
            for c in refused:
                assert mw.expected_status("weighted", c) == UNSUPPORTED, c
    # weights a float cannot hold: only the float V-cycle refuses them
    assert mw.expected_status("weighted", config("f32", op="big")) == UNSUPPORTED
    for c in (config(op="big"), config(channels="batched", op="big"), config(smoother="line", op="big")):
        assert mw.expected_status("weighted", c) == OK, c
    # no operator: a call sequence error in every mode, refused ones included
    for precision in ("f64", "f32"):
        for channels in ("sequential", "batched"):
            for smoother in ("point", "line"):
                assert mw.expected_status("weighted", config(precision, channels, smoother, op=None)) == STATE
    # the line smoother serves weighted handles only
    for kind, op in (("structured", "S"), ("mask", "M"), ("mask", "Mc")):
        assert mw.expected_status(kind, config(op=op)) == OK
        assert mw.expected_status(kind, config("f32", op=op)) == OK
        assert mw.expected_status(kind, config(channels="batched", op=op)) == OK
        assert mw.expected_status(kind, config(smoother="line", op=op)) == UNSUPPORTED
        assert mw.expected_status(kind, config("f32", "batched", op=op)) == UNSUPPORTED


def test_served_modes_and_refusal_reasons():
    assert len(mw.served_modes("weighted")) == 8 and len(mw.served_modes("mask")) == 3 and len(mw.served_modes("structured")) == 3
    assert ("f64", "sequential", "line", "rescaled") in mw.served_modes("weighted")
    assert all(m[2] == "point" for m in mw.served_modes("mask"))
    assert mw.reasons("weighted", config("f32", "batched", "line", op=None)) == ("no_operator", "batched_f32", "line_f32", "line_batched")
    assert mw.reasons("mask", config(smoother="line", op="M")) == ("line_not_weighted",)


def test_apply_step():
    c = mw.START["weighted"]
    c, status = mw.apply_step("weighted", c, ("precision", "f32"))
    assert status == OK and c == config("f32")
    c, status = mw.apply_step("weighted", c, ("hierarchy", "rescaled"))
    assert status == OK and c == config("f32", hierarchy="rescaled")
    c, status = mw.apply_step("weighted", c, ("weights", "nan"))
    assert status == BAD_ARG and c == config("f32", hierarchy="rescaled", op=None)      # the modes survive, the operator does not
    c, status = mw.apply_step("weighted", c, ("weights", "Bfixed"))
    assert status == OK and c == config("f32", hierarchy="rescaled", op="Bfixed")
    for kind in ("structured", "mask"):                            # the hierarchy kind is a weighted handle's
        c, status = mw.apply_step(kind, mw.START[kind], ("hierarchy", "rescaled"))
        assert status == UNSUPPORTED and c == mw.START[kind]
    c, status = mw.apply_step("mask", mw.START["mask"], ("mask", "Mc"))
    assert status == OK and c[4] == "Mc"
    with pytest.raises(ValueError):
        mw.apply_step("structured", mw.START["structured"], ("weights", "A"))


@pytest.mark.parametrize("kind", mw.KINDS)
def test_the_committed_walk_reaches_everything(kind):
    seed, n = mw.WALKS[kind]
    assert 0 < n <= 64
    steps = mw.walk(kind, seed, n)
    assert len(steps) == n and steps == mw.walk(kind, seed, n)      # seeded: the same sequence every time
    assert set(steps) <= set(mw.alphabet(kind))
    missing = mw.coverage(kind, steps)
    seen = mw.configs(kind, steps)
    print(f"{kind}: seed {seed}, {n} steps, {len({c for _, c, _, _ in seen})} configurations, "
          f"{sum(not mw.reasons(kind, c) for _, c, _, _ in seen)} served solves, the last one {seen[-1][1]}")
    assert missing == {"steps": [], "modes": [], "refusals": []}, missing


@pytest.mark.parametrize("kind", mw.KINDS)
def test_coverage_notices_a_walk_that_falls_short(kind):
    seed, n = mw.WALKS[kind]
    steps = mw.walk(kind, seed, n)
    short = mw.coverage(kind, steps[:4])
    assert short["steps"] and short["modes"] and short["refusals"]
    # without the steps that change the operator nothing is reached "directly after an operator change"
    if kind != "structured":
        quiet = [s for s in steps if s not in mw.operator_steps(kind)]
        assert mw.coverage(kind, quiet)["modes"] == mw.served_modes(kind)
    # a walk that ends in its only refusal never recovers from it
    lone = [("smoother", "line"), ("precision", "f32"), ("smoother", "point"), ("channels", "batched")]
    assert "batched_f32" in mw.coverage(kind, lone)["refusals"]
