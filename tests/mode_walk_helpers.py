"""Test-side model of the multigrid mode switches of a grid handle (include/ccp_gs.h: ccp_grid_mg_set_precision,
_set_channels, _set_smoother, _set_hierarchy, ccp_grid_set_weights_*, ccp_grid_set_mask_host), NOT product code.  Pure
Python: no GPU, no numpy.

A configuration is the tuple (precision, channels, smoother, hierarchy, operator id) of a handle of one kind
("structured", "mask", "weighted").  Operator ids: "S" (a structured handle's own matrix), "M" / "Mc" (a mask and its
complement), "A" / "B" (two sets of random weights), "Afixed" / "Bfixed" (the same weights with 10 % fixed pixels), "big"
(3e38 weights: float32-finite, but their sums are not), None (no operator: the last set_weights was refused).

* `expected_status(kind, config)`: what ccp_grid_mg_apply and ccp_grid_mg_conjugate_gradient must return, written from
  the header's contract;
* `reasons(kind, config)`: every refusal reason that holds in a configuration;
* `apply_step(kind, config, step)`: the configuration after a setter call and the status the setter must return;
* `walk(kind, seed, steps)`: a seeded sequence of steps (the generator is written out below, so the sequence does not
  depend on a library's random stream);
* `coverage(kind, steps)`: what a walk reaches; tests/test_mode_walk_helpers.py holds the committed walks (WALKS) to it.
"""

OK, BAD_ARG, STATE, UNSUPPORTED = 0, 1, 5, 6
KINDS = ("structured", "mask", "weighted")
START = {"structured": ("f64", "sequential", "point", "galerkin", "S"),
         "mask": ("f64", "sequential", "point", "galerkin", "M"),
         "weighted": ("f64", "sequential", "point", "galerkin", "A")}
MODE_STEPS = [("precision", "f64"), ("precision", "f32"), ("channels", "sequential"), ("channels", "batched"),
              ("smoother", "point"), ("smoother", "line"), ("hierarchy", "galerkin"), ("hierarchy", "rescaled")]
WEIGHT_STEPS = [("weights", "A"), ("weights", "B"), ("weights", "Bfixed"), ("weights", "big"), ("weights", "nan")]
MASK_STEPS = [("mask", "M"), ("mask", "Mc")]
# the committed walks: kind -> (seed, steps); at most 64 steps per handle kind
WALKS = {"structured": (12, 24), "mask": (412, 40), "weighted": (58, 64)}


def reasons(kind, config):
    """Every reason the contract gives for refusing a solve in `config`, as a tuple of names (empty: served)."""
    precision, channels, smoother, _, op = config
    out = []
    if op is None:
        out.append("no_operator")
    if channels == "batched" and precision == "f32":
        out.append("batched_f32")
    if smoother == "line":
        if kind != "weighted":
            out.append("line_not_weighted")
        if precision == "f32":
            out.append("line_f32")
        if channels == "batched":
            out.append("line_batched")
    if precision == "f32" and op == "big":
        out.append("f32_unholdable")
    return tuple(out)


def expected_status(kind, config):
    why = reasons(kind, config)
    if not why:
        return OK
    return STATE if "no_operator" in why else UNSUPPORTED     # the call sequence is judged before the modes


def alphabet(kind):
    return MODE_STEPS + (WEIGHT_STEPS if kind == "weighted" else MASK_STEPS if kind == "mask" else [])


def operator_steps(kind):
    """The steps that can change the operator of the V-cycle: the weights or the mask, and a weighted handle's hierarchy kind."""
    if kind == "weighted":
        return WEIGHT_STEPS + [s for s in MODE_STEPS if s[0] == "hierarchy"]
    return MASK_STEPS if kind == "mask" else []


def apply_step(kind, config, step):
    """(the configuration after `step`, the status the setter returns)"""
    precision, channels, smoother, hierarchy, op = config
    name, arg = step
    if name == "precision":
        return (arg, channels, smoother, hierarchy, op), OK
    if name == "channels":
        return (precision, arg, smoother, hierarchy, op), OK
    if name == "smoother":
        return (precision, channels, arg, hierarchy, op), OK
    if name == "hierarchy":                                    # weighted handles only; the others keep GALERKIN
        if kind != "weighted":
            return config, UNSUPPORTED
        return (precision, channels, smoother, arg, op), OK
    if name == "weights" and kind == "weighted":
        if arg == "nan":                                       # refused, and the handle is left with no operator
            return (precision, channels, smoother, hierarchy, None), BAD_ARG
        return (precision, channels, smoother, hierarchy, arg), OK
    if name == "mask" and kind == "mask":
        return (precision, channels, smoother, hierarchy, arg), OK
    raise ValueError((kind, step))


def served_modes(kind):
    """Every (precision, channels, smoother, hierarchy) the contract serves on a handle of `kind` with a holdable operator."""
    out = []
    for hierarchy in (("galerkin", "rescaled") if kind == "weighted" else ("galerkin",)):
        for precision in ("f64", "f32"):
            for channels in ("sequential", "batched"):
                for smoother in ("point", "line"):
                    if not reasons(kind, (precision, channels, smoother, hierarchy, "A")):
                        out.append((precision, channels, smoother, hierarchy))
    return out


def refusal_reasons(kind):
    out = ["batched_f32"]
    out += ["line_f32", "line_batched", "f32_unholdable", "no_operator"] if kind == "weighted" else ["line_not_weighted"]
    return out


class _Lcg:
    """Knuth's 64-bit linear congruential generator, the high 32 bits of every state."""

    def __init__(self, seed):
        self.x = (seed * 2654435761 + 1) & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return ((self.x >> 32) * n) >> 32


def walk(kind, seed, steps):
    """`steps` steps of the alphabet of `kind`: an operator step or a mode step with equal chance (a structured handle
    has mode steps only), uniform within either group."""
    g = _Lcg(seed)
    ops = operator_steps(kind)
    out = []
    for _ in range(steps):
        group = ops if ops and g.below(2) else MODE_STEPS
        out.append(group[g.below(len(group))])
    return out


def configs(kind, steps):
    """[(step, configuration after it, setter status, whether the step changed the operator of the V-cycle)]"""
    config = START[kind]
    out = []
    for step in steps:
        after, status = apply_step(kind, config, step)
        changed = after[3:] != config[3:]                      # (setting the current hierarchy, weights or mask again: no)
        out.append((step, after, status, changed))
        config = after
    return out


def coverage(kind, steps):
    """What the walk misses of: every step kind twice, every served mode directly after an operator change (a structured
    handle, which has none: reached at all), every refusal reason alone in a configuration and followed later by a
    served solve.  A dict of three lists, all empty when nothing is missing."""
    seen = configs(kind, steps)
    counts = {s: 0 for s in alphabet(kind)}
    for step, _, _, _ in seen:
        counts[step] += 1
    after_change = set()
    for _, config, _, changed in seen:
        if (changed or kind == "structured") and not reasons(kind, config):
            after_change.add(config[:4])
    recovered = set()
    for i, (_, config, _, _) in enumerate(seen):
        why = reasons(kind, config)
        if len(why) == 1 and any(not reasons(kind, later[1]) for later in seen[i + 1:]):
            recovered.add(why[0])
    return {"steps": [s for s in alphabet(kind) if counts[s] < 2],
            "modes": [m for m in served_modes(kind) if m not in after_change],
            "refusals": [r for r in refusal_reasons(kind) if r not in recovered]}
