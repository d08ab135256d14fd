"""CPU: the fp64 clip + Adam reference of tests/ref64_optim.py held to torch's own float64 optimizer, the condition on the inputs of every
case the GPU tests use, where the margins of tests/test_optim_fp64_gpu.py come from (a second correct fp32 formulation against the CPU's
yardstick), and which wrong formulas the bars reject.  Run with ``-s`` for the figures DESIGN 2.2 quotes."""
import collections

import pytest
import torch

from tests import ref64_optim as R

SIZES = (1, 3, 257, 1025, 17101)


def _grid(sizes, clip_fracs=(1, 3)):
    """The whole regime grid at every size, clip_n = n and n // 3, grad_scale cycling through 1, 1/2, 1/3: 144 draws per size."""
    for n in sizes:
        for i, (gs, st, lr, p0) in enumerate(R.regime_grid()):
            for j, d in enumerate(clip_fracs):
                yield (gs, st, lr, p0), R.build(n, gs, st[0], st[1], lr, p0, n // d, R.GRAD_SCALES[(i + j) % 3], R.case_seed(n, i, j))


def test_reference_equals_torch_float64_clip_and_adam():
    """``reference(rounded=False)`` against ``clip_grad_norm_`` + ``torch.optim.Adam`` in float64 over every regime and
    clip_n in {n, n // 3, 0}: 1e-13 on the metric the kernels are judged on."""
    worst = collections.defaultdict(float)
    count = 0
    for n in (257, 1025):
        for i, (gs, st, lr, p0) in enumerate(R.regime_grid()):
            for j, clip_n in enumerate((n, n // 3, 0)):
                case = R.build(n, gs, st[0], st[1], lr, p0, clip_n, R.GRAD_SCALES[(i + j) % 3], R.case_seed(n, i, j))
                ref = R.reference_of(case, rounded=False)
                got = R.torch_run(case, "cpu", torch.float64, rounded=False)
                for q, x in R.metrics(got, ref).items():
                    worst[q] = max(worst[q], x)
                    assert x <= 1e-13, (case["id"], q, x)
                count += 1
    print(f"\nreference vs torch float64 over {count} draws: " + ", ".join(f"{q} {x:.2e}" for q, x in worst.items()))


def test_every_gpu_case_meets_the_input_condition():
    """Every non-zero g, gc, v0, v and g^2 (1 - beta2) in fp32's normal range, sum g^2 below fp32's maximum -- re-asserted here for the
    synthetic cases of tests/test_optim_fp64_gpu.py (``build`` asserts it too; the chained-tail test asserts it for its real gradient)."""
    cases = [R.build(**kw) for kw in R.K6B_CASES + R.K6_CASES]
    for pol in R.APPLY_POLICIES:
        n = R.policy_n_params(*pol)
        cases += [R.build(n=n, **kw) for kw in R.apply_cases(pol)] + [R.build(n=n, **kw) for kw, _parts in R.parts_cases(pol)]
    for case in cases:
        R.assert_input_condition(case)
    sizes = sorted({c["n"] for c in cases})
    assert {1, 3, 255, 256, 257, 1023, 1025, 17101, 524288 + 1025} <= set(sizes)
    for n in (17101, 524288 + 1025):         # every regime value at the 2 x 64 bucket and at the largest size
        at = [kw for kw in R.K6B_CASES if kw["n"] == n]
        assert {kw["gscale"] for kw in at} == set(R.GSCALES) and {(kw["state"], kw["t"]) for kw in at} == set(R.STATES)
        assert {kw["lr"] for kw in at} == set(R.LRS) and {kw["p0_kind"] for kw in at} == set(R.P0S)
        assert {kw["clip_n"] for kw in at} == {n, n // 3, 1, 0}
    print(f"\n{len(cases)} synthetic GPU cases meet the input condition; sizes {sizes}")


def test_margins_come_from_a_second_correct_fp32_formulation():
    """``replay_fp32`` (adam_math.h's operation order in numpy float32) against the CPU's Y over the whole regime grid at five sizes
    (720 draws).  The margin of a quantity is the worst ratio rounded up to the next power of two; ``norm``, whose worst is the
    half-ulp limit itself (0.9998 of a floored Y), takes 2 so that the bar is not decided at the 2^-53 level (a correctly rounded
    fp64 square root rounded again to fp32).  Nothing here comes from the GPU kernels."""
    worst, where, count = collections.defaultdict(float), {}, 0
    for _reg, case in _grid(SIZES):
        ref = R.reference_of(case)
        Y, _ = R.yardstick(case, ref, "cpu")
        for q, x in R.metrics(R.replay_fp32(case), ref).items():
            if x / Y[q] > worst[q]:
                worst[q], where[q] = x / Y[q], case["id"]
        count += 1
    assert count >= 600
    print(f"\nreplay_fp32 against the CPU yardstick over {count} draws, worst ratio per quantity:")
    for q in R.QUANTITIES:
        print(f"  {q:5s} {worst[q]:5.2f} x Y  (margin {R.MARGINS[q]:g})  at {where[q]}")
    for q in R.QUANTITIES:
        assert worst[q] <= R.MARGINS[q], (q, worst[q], where[q])


# mutant -> (the regime in which it is a different computation and must be rejected, in words; the same as a predicate)
_t_small = lambda reg, case: reg[1][1] <= 1000                                                          # noqa: E731
_active = lambda reg, case: reg[0] in ("active", "edge") and case["clip_n"] > 0                         # noqa: E731
APPLIES = collections.OrderedDict([
    ("no_1e6", ("gradient scale 'edge' (norm = 1.5 max_norm)", lambda reg, case: reg[0] == "edge")),
    ("clip_past_clip_n", ("clip active and clip_n < n", lambda reg, case: _active(reg, case) and case["clip_n"] < case["n"])),
    ("t_minus_1", ("t <= 1000", _t_small)),
    ("pow_f32", ("t <= 1000 with the step visible in p (lr = 1 or p0 = 0)", lambda reg, case: _t_small(reg, case) and (reg[2] == 1.0 or reg[3] == "zero"))),
    ("eps_inside_bc2", ("t <= 1000 (at t = 100000 sqrt(bc2) rounds to 1)", _t_small)),
    ("sqrt_v_plus_eps2", ("everywhere", lambda reg, case: True)),
    ("no_bc2", ("t <= 1000", _t_small)),
    ("m_unclipped", ("clip active", _active)),
    ("v_unclipped", ("clip active", _active)),
    ("grad_scale_twice", ("grad_scale != 1", lambda reg, case: case["grad_scale"] != 1.0)),
])
_MUTANT_DRAWS = {}


def _mutant_draws():
    if not _MUTANT_DRAWS:
        _MUTANT_DRAWS["d"] = []
        for reg, case in _grid((1025, 17101)):
            ref = R.reference_of(case)
            _MUTANT_DRAWS["d"].append((reg, case, ref, R.yardstick(case, ref, "cpu")[0]))
    return _MUTANT_DRAWS["d"]


@pytest.mark.parametrize("mutant", list(APPLIES))
def test_the_bars_reject_a_wrong_formula(mutant):
    """Each wrong variant of ``replay_fp32`` must exceed the margin on at least one quantity in EVERY draw of the regime where it
    applies (n = 1025 and 17101, clip_n = n and n // 3: 288 draws).  Prints metric / (margin * Y) of every draw and quantity (> 1 is a rejection), then
    per quantity its range over the regime, and how many draws outside the regime happen to be rejected as well."""
    assert set(APPLIES) == set(R.MUTANTS)
    words, applies = APPLIES[mutant]
    lo, hi = collections.defaultdict(lambda: float("inf")), collections.defaultdict(float)
    n_in = n_out = rej_out = 0
    low_best, missed, lines = float("inf"), [], []
    for reg, case, ref, Y in _mutant_draws():
        over = {q: x / (R.MARGINS[q] * Y[q]) for q, x in R.metrics(R.replay_fp32(case, mutant), ref).items()}
        best = max(over.values())
        lines.append(f"  {'in ' if applies(reg, case) else 'out'} " + " ".join(f"{q} {x:9.3g}" for q, x in over.items()) + f"  {case['id']}")
        if applies(reg, case):
            n_in += 1
            for q, x in over.items():
                lo[q], hi[q] = min(lo[q], x), max(hi[q], x)
            low_best = min(low_best, best)
            if not best > 1.0:
                missed.append((case["id"], over))
        else:
            n_out += 1
            rej_out += best > 1.0
    print(f"\n{mutant}: metric / (margin * Y) per draw and quantity ('in': a draw of the regime where it applies)\n" + "\n".join(lines))
    print(f"\n{mutant}: applies in [{words}], {n_in} draws; worst quantity over its bar: lowest {low_best:.3g} x; per quantity "
          + ", ".join(f"{q} {lo[q]:.3g}..{hi[q]:.3g}" for q in R.QUANTITIES) + f"; outside the regime {rej_out} of {n_out} draws rejected")
    assert n_in > 0 and not missed, (mutant, len(missed), missed[:2])
