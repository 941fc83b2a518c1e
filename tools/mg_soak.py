#!/usr/bin/env python3
"""Differential soak of the multigrid PCG family (GPU): the cases of tests/mg_soak_cases.py -- random shapes at the tile,
tail and lane-count edges, every served mode, every operator and mask class -- against the numpy models of
tests/*_helpers.py and an independent direct solve.

    tools/mg_soak.py N SEED [--checks ABCDE] [--progress K] [--stats FILE]
    tools/mg_soak.py --committed                  (the runs and the regressions tests/test_gpu_mg_soak.py goes through)
    tools/mg_soak.py --case "Case(kind=...)"

Per case:
  A  mg_levels(ch) of every channel equals the model hierarchy;
  B  one V-cycle, mg_apply(nu) on a random b: the point smoother (f64, f32) equals the model; batched channels also hold
     the sequential call's bits; the line smoother is within 16 x line_helpers.deviation of the model; "constant" mode is
     the projected V-cycle on an integer b, within the rounding of one mean;
  C  the synchronous PCG at epsilon = 1e-10 |b of channel 0| and a cap of the model's count + 3: every channel converges,
     and x is within 16 x the model PCG's own distance from a direct solve (scipy spsolve of a matrix assembled here from
     the header's formulas; a distance under one ulp of the solution's largest value counts as that ulp); a floating
     system is compared mean-free;
  D  on a twin handle, the enqueue solve equals C's x and report bit for bit, and the relative enqueue solve
     (epsilon_abs 0, epsilon_rel 1e-8) equals the synchronous call at the threshold it reports;
  E  weighted operators without fixed pixels: refresh_weights_tensor to a second operator of the class, then A, and the
     enqueue solve against the synchronous solve of a fresh handle built with that operator, bit for bit.

A mismatch is one line -- the check's letter, the case's repr, the largest difference -- and exit status 1.  Anything else
that goes wrong (a HIP error, a CcpError: the generator emits served configurations only) ends the run at once with exit
status 2: nothing more is started on the GPU after it."""
import argparse
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mg_soak_cases as sc  # noqa: E402

FACTOR = 16.0                     # tests/test_gpu_mg_line.py's and tests/test_gpu_adjoint.py's
REL = 1e-8
SENTINEL = -7.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def maxdiff(a, b):
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


class Soak:
    def __init__(self, checks="ABCDE", out=print):
        import torch
        from coursecomputationalphotography_amd import capi
        self.torch, self.capi, self.dev = torch, capi, torch.device("cuda", 0)
        self.checks, self.out = checks, out
        self.mismatches = []
        self.stats = {}            # class -> largest count difference, model and device distance at the largest ratio

    def report(self, letter, case, diff, what=""):
        line = f"{letter} {case!r} {diff:.6e}" + (f" [{what}]" if what else "")
        self.mismatches.append(line)
        self.out(line)

    # ---- handles -------------------------------------------------------------------------------------------------------
    def stacked(self, ops, i):
        return self.torch.from_numpy(np.stack([op[i] for op in ops], axis=-1)).to(self.dev)

    def make(self, case, ops):
        """A fresh handle in the case's modes holding `ops`: the modes first, then the operator."""
        capi = self.capi
        if case.kind == "weighted":
            g = capi.Grid(case.W, case.H, case.C, weighted=True)
            g.mg_configure(hierarchy=case.hierarchy, precision=case.precision, channels=case.channels, smoother=case.smoother,
                           nullspace=case.nullspace)
            if case.op == "per_channel":
                g.set_weights_per_channel_tensor(*(self.stacked(ops, i) for i in range(3)))
            else:
                wx, wy, lam, fixed = ops[0]
                g.set_weights(wx, wy, lam, fixed=fixed)
            return g
        g = capi.Grid(case.W, case.H, case.C) if case.kind == "structured" else capi.Grid(case.W, case.H, case.C, mask=ops[0])
        g.mg_configure(precision=case.precision, channels=case.channels, smoother=case.smoother)
        return g

    @staticmethod
    def load(g, m):
        for c in range(g.C):
            g.set_b(m.b[c], c)
            g.set_x(m.x0[c], c)

    # ---- the checks ----------------------------------------------------------------------------------------------------
    def levels(self, g, m, letter="A"):
        case = m.case
        for c in range(case.C):
            got, want = g.mg_levels(c), m.levels[c]
            if len(got) != len(want):
                self.report(letter, case, float(abs(len(got) - len(want))), f"channel {c}: {len(got)} levels, the model {len(want)}")
                continue
            for k, (have, lv) in enumerate(zip(got, want)):
                for name, a, b in zip(("d", "we", "ws"), have, lv.coefficients()):
                    if a.shape != b.shape or not np.array_equal(a, b):
                        self.report(letter, case, maxdiff(a, b) if a.shape == b.shape else float("inf"), f"channel {c} level {k} {name}")

    def apply(self, g, m):
        case = m.case
        for c in range(case.C):
            g.set_b(m.vb[c], c)
        g.fill_x(123.0)
        sequential = None
        if case.channels == "batched":
            g.mg_set_channels("sequential")
            g.mg_apply(case.nu)
            sequential = [g.get_x(c) for c in range(case.C)]
            g.mg_set_channels("batched")
            g.fill_x(123.0)
        g.mg_apply(case.nu)
        for c in range(case.C):
            got = g.get_x(c)
            want, z, dev = sc.model_vcycle(m, c)
            if not np.array_equal(bits(g.get_b(c)), bits(m.vb[c])):
                self.report("B", case, maxdiff(g.get_b(c), m.vb[c]), f"channel {c}: b after mg_apply")
            if sequential is not None and not np.array_equal(bits(got), bits(sequential[c])):
                self.report("B", case, maxdiff(got, sequential[c]), f"channel {c}: batched against sequential")
            if case.nullspace == "constant":
                bound = 2 * z.size * 2.0 ** -53 * float(np.abs(z).max())     # the rounding of one n-term sum (tests/test_gpu_neumann.py)
                if dev is not None:
                    bound += FACTOR * dev * float(np.abs(z).max())
                err = maxdiff(got, want)
                if not (np.all(np.isfinite(got)) and err <= bound):
                    self.report("B", case, err, f"channel {c}: projected V-cycle, bound {bound:.3e}")
            elif dev is not None:
                scale = float(np.max(np.abs(want)))
                err = maxdiff(got, want) / scale if scale else maxdiff(got, want)
                if not (np.all(np.isfinite(got)) and err <= FACTOR * dev):
                    self.report("B", case, err, f"channel {c}: line V-cycle, bound {FACTOR * dev:.3e}")
            elif not np.array_equal(got, want):
                self.report("B", case, maxdiff(got, want), f"channel {c}: V-cycle")

    def solve(self, g, m):
        """C: (x per channel, the reports, the cap)"""
        case = m.case
        models = [sc.model_pcg(m, c, 200) for c in range(case.C)]
        cap = max(r[1] for r in models) + 3
        self.load(g, m)
        reps = g.mg_conjugate_gradient(m.eps, cap, case.nu)
        xs = [g.get_x(c) for c in range(case.C)]
        st = self.stats.setdefault(case.op, dict(cases=0, channels=0, same_bits=0, count_diff=0, ratio=0.0, model=0.0, device=0.0))
        st["cases"] += 1
        st["channels"] += case.C
        st["same_bits"] += sum(bool(np.array_equal(bits(xs[c]), bits(models[c][0]))) for c in range(case.C))   # (a figure, not a check)
        for c in range(case.C):
            if not reps[c].converged:
                self.report("C", case, float(reps[c].last_l1_step), f"channel {c}: not converged in {cap}, the model in {models[c][1]}")
                continue
            if abs(reps[c].iterations - models[c][1]) > abs(st["count_diff"]):
                st["count_diff"] = reps[c].iterations - models[c][1]
            ref, solved = sc.direct(m, c)
            dm, dd = sc.distance(m, c, models[c][0], ref, solved), sc.distance(m, c, xs[c], ref, solved)
            # The reference is itself a float64: no distance from it is known to less than an ulp of its largest value.
            # Isolated pixels (a checkerboard mask: A = 4 I) put the model exactly on it, and the device, whose dot
            # products add up in another order, one ulp away.
            dm = max(dm, float(np.spacing(np.max(np.abs(ref)))))
            if dd / dm > st["ratio"]:
                st.update(ratio=dd / dm, model=dm, device=dd)
            if not (np.all(np.isfinite(xs[c])) and dd <= FACTOR * dm):
                self.report("C", case, dd, f"channel {c}: |x - direct|, the model's {dm:.3e}")
        return xs, reps, cap

    def report_tensor(self, C, fields):
        return self.torch.full((C, fields), SENTINEL, dtype=self.torch.float64, device=self.dev)

    def same_solve(self, letter, case, g, want_x, reps, rep, ref_handle, what, channels=None):
        """x and the report of an enqueue solve (g, rep: the report's rows) against a synchronous one."""
        for c in (range(case.C) if channels is None else channels):
            x = g.get_x(c)
            if not np.array_equal(bits(x), bits(want_x[c])):
                self.report(letter, case, maxdiff(x, want_x[c]), f"channel {c}: {what}, x")
            want = [float(reps[c].iterations), float(reps[c].converged), reps[c].last_l1_step, 0.0, 0.0, 0.0]
            if case.nullspace == "constant":
                want[3], want[4], _ = ref_handle.mg_nullspace_info(c)
            if not np.array_equal(bits(rep[c, :6]), bits(np.array(want))):
                self.report(letter, case, maxdiff(rep[c, :6], want), f"channel {c}: {what}, report {rep[c, :6].tolist()} against {want}")

    def enqueue(self, g, m, xs, reps, cap):
        """D, on a twin handle; returns the twin, prepared (E goes on with it)."""
        case, torch = m.case, self.torch
        twin = self.make(case, m.ops)
        self.load(twin, m)
        twin.mg_prepare(case.nu)
        rep = self.report_tensor(case.C, 6)
        twin.mg_conjugate_gradient_enqueue(m.eps, cap, case.nu, rep)
        torch.cuda.synchronize()
        self.same_solve("D", case, twin, xs, reps, rep.cpu().numpy(), g, "enqueue")
        self.load(twin, m)
        rep = self.report_tensor(case.C, 8)
        twin.mg_conjugate_gradient_enqueue_relative(0.0, REL, cap, case.nu, rep)
        torch.cuda.synchronize()
        rep = rep.cpu().numpy()
        for c in range(case.C):
            self.load(g, m)
            sync = g.mg_conjugate_gradient(float(rep[c, 7]), cap, case.nu)
            self.same_solve("D", case, twin, [g.get_x(k) for k in range(case.C)], sync, rep, g, "relative enqueue", channels=[c])
        return twin

    def refresh(self, twin, case, cap):
        """E, on D's twin."""
        torch = self.torch
        m2 = sc.cached(case, 1)
        if case.op == "per_channel":
            w = [self.stacked(m2.ops, i) for i in range(3)]
        else:
            w = [torch.from_numpy(a).to(self.dev) for a in m2.ops[0][:3]]
        twin.refresh_weights_tensor(*w)
        status = twin.operator_status()
        if status != 0:
            self.report("E", case, float(status), "operator_status after the refresh")
            return
        self.levels(twin, m2, "E")
        fresh = self.make(case, m2.ops)
        self.load(fresh, m2)
        reps = fresh.mg_conjugate_gradient(m2.eps, cap, case.nu)
        self.load(twin, m2)
        rep = self.report_tensor(case.C, 6)
        twin.mg_conjugate_gradient_enqueue(m2.eps, cap, case.nu, rep)
        torch.cuda.synchronize()
        self.same_solve("E", case, twin, [fresh.get_x(c) for c in range(case.C)], reps, rep.cpu().numpy(), fresh, "enqueue after the refresh")
        fresh.close()

    def one(self, case):
        m = sc.cached(case)
        g = self.make(case, m.ops)
        if "B" in self.checks:
            self.apply(g, m)
        if "A" in self.checks:
            self.levels(g, m)
        if "C" in self.checks:
            xs, reps, cap = self.solve(g, m)
            if "D" in self.checks:
                twin = self.enqueue(g, m, xs, reps, cap)
                if "E" in self.checks and case.kind == "weighted" and case.op != "fixed":
                    self.refresh(twin, case, cap)
                twin.close()
        g.close()


def run(cases, checks="ABCDE", out=print, stats=None, progress=0):
    """Every case through the checks named in `checks`: the list of mismatch lines (each also given to `out`).  An exception
    that is not a mismatch is not caught.  stats: a dict that receives, per operator class, the largest difference of the
    device's iteration count from the model's and the distances from the direct solve at the largest ratio."""
    soak = Soak(checks, out)
    for i, case in enumerate(cases):
        if progress and i and i % progress == 0:
            out(f"mg_soak: {i} of {len(cases)} cases, {len(soak.mismatches)} mismatches")
        try:
            soak.one(case)
        except BaseException:
            out(f"X {case!r}")                                        # which case it was; the caller sees the exception itself
            raise
    soak.torch.cuda.synchronize()
    if stats is not None:
        stats.update(soak.stats)
    return soak.mismatches


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("seed", nargs="?", type=int)
    ap.add_argument("--case", action="append", help="the repr of one case (may be given more than once)")
    ap.add_argument("--committed", action="store_true", help="the committed runs and the regressions of tests/mg_soak_cases.py")
    ap.add_argument("--checks", default="ABCDE")
    ap.add_argument("--progress", type=int, default=0, help="a line every so many cases")
    ap.add_argument("--stats", help="write the per-class figures of check C to this JSON file")
    args = ap.parse_args(argv)
    if args.case:
        todo = [sc.case_from_repr(line) for line in args.case]
    elif args.committed:
        todo = sc.committed_cases() + [sc.case_from_repr(line) for line in sc.REGRESSIONS]
    elif args.n is not None and args.seed is not None:
        todo = sc.cases(args.seed, args.n)
    else:
        ap.error("N SEED, --committed or --case")
    stats, t0 = {}, time.time()
    try:
        bad = run(todo, args.checks, lambda line: print(line, flush=True), stats, args.progress)
    except BaseException:                                             # not a mismatch: stop here, start nothing more
        traceback.print_exc()
        print(f"mg_soak: stopped by an exception after {time.time() - t0:.1f} s", flush=True)
        return 2
    print(f"mg_soak: {len(todo)} cases, checks {args.checks}, {len(bad)} mismatches, {time.time() - t0:.1f} s", flush=True)
    for name, st in sorted(stats.items()):
        print(f"  {name}: {st['cases']} cases, x equals the model's bits on {st['same_bits']} of {st['channels']} channels, "
              f"count - model {st['count_diff']:+d}, largest device/model distance {st['ratio']:.3g} "
              f"(model {st['model']:.3e}, device {st['device']:.3e})", flush=True)
    if args.stats:
        with open(args.stats, "w") as f:
            json.dump(stats, f, indent=1, sort_keys=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
