"""CPU: the fp64 loss reference of tests/ref64_loss.py pinned to the golden fixtures and to the C oracle, the condition on the inputs of every
case the GPU tests use, where the margins of tests/test_loss_fp64_gpu.py come from (a numpy-float32 replay of loss.hip against the CPU's
yardstick; it never sees a kernel), and which wrong variants of that replay the bars reject.  Run with ``-s`` for the figures DESIGN 2.3
quotes."""
import collections

import numpy as np
import pytest
import torch

from tests import ref64_loss as R
from tests.util import load

# M classes of the derivation: below TINY_M, around a wave / a workgroup / the 1024-sample block, and (fewer draws) the strided fold
M_TINY = (1, 2, 3, 17, 30)
M_CLASSES = (31, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
M_LARGE = (262145,)            # every regime, the hyperparameter set rotating
M_HUGE = (2095109,)            # the normal regime once: the grid-stride loop's third trip


def _x_of(a):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(a[k], dtype=np.float32).reshape(-1))          # noqa: E731
    return dict(newlogp=t("newlogp"), newv=t("newv"), entropy=t("entropy"), rec=torch.stack([t("oldlogp"), t("adv"), t("ret"), t("oldv")], 1))


def test_reference_equals_golden_fixtures_and_c_oracle():
    """``run_terms`` in float64 against tests/golden/loss.npz and against ``oracle.c_oracle.ppo_loss`` on the distribution of
    test_hip_parity.py::test_loss_vs_c_oracle, at the tolerances the GPU tests use for the kernel against them."""
    from oracle import c_oracle as CO
    z = load("loss.npz")
    for name in z["names"]:
        T, N, norm_adv, clip_vloss, clip, ec, vc = z[f"{name}/meta"]
        x = _x_of({k: z[f"{name}/{k}"] for k in ("newlogp", "oldlogp", "adv", "newv", "oldv", "ret", "entropy")})
        # the two "boundary" fixtures put samples ON a decision in fp32 (a ratio or a value step that equals its edge): there the same
        # ``loss_terms`` is pinned in float32, where those decisions are the fixture's; every other fixture in float64
        dtype = torch.float32 if "boundary" in str(name) else torch.float64
        ref = R.run_terms(x, dict(clip=float(clip), ent_coef=float(ec), vf_coef=float(vc)), bool(norm_adv), 1 if clip_vloss else 2, dtype)
        np.testing.assert_allclose(ref["scalars"].numpy()[[1, 2, 3, 4, 5, 6]], z[f"{name}/scalars"], rtol=1e-5, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(ref["g_newlogp"].numpy(), z[f"{name}/g_newlogp"], rtol=1e-5, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(ref["g_newv"].numpy(), z[f"{name}/g_newv"], rtol=1e-5, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(ref["g_entropy"].numpy(), z[f"{name}/g_entropy"], rtol=1e-6, err_msg=name)
    for M in (2, 63, 1000, 16384):
        x = R.build_inputs(M)
        rec = x["rec"].numpy()
        for na, vm in R.COMBOS:
            ref = R.run_terms(x, R.HYPERS[0], na, vm)
            sc, g_lp, g_v, g_e = CO.ppo_loss(x["newlogp"].numpy(), rec[:, 0], rec[:, 1], x["newv"].numpy(), rec[:, 3], rec[:, 2],
                                             x["entropy"].numpy(), 0.2, 0.01, 0.5, bool(na), vm)
            np.testing.assert_allclose(sc, ref["scalars"].numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(g_lp, ref["g_newlogp"].numpy(), rtol=1e-5, atol=1e-10)      # branch-safe inputs: no sample forgiven
            np.testing.assert_allclose(g_v, ref["g_newv"].numpy(), rtol=1e-5, atol=1e-10)
            np.testing.assert_allclose(g_e, ref["g_entropy"].numpy(), rtol=1e-6)


def test_every_case_is_branch_safe_and_the_regimes_are_what_they_say():
    """``build_inputs`` asserts that zero samples lie within BRANCH_EPS of a decision; here for every (regime, hyperparameter set) at the
    sizes the GPU regime test uses, with what each regime promises about its inputs."""
    for M in (65, 1025, 262145):
        for regime in R.REGIMES:
            for hi, h in enumerate(R.HYPERS):
                x = R.build_inputs(M, regime, hi)
                R.assert_safe(x, h["clip"])
                rec = x["rec"].double()
                adv, lr, dv = rec[:, 1], x["newlogp"].double() - rec[:, 0], x["newv"].double() - rec[:, 3]
                if regime == "offset":
                    assert 80 < float(adv.mean() / adv.std()) < 125
                if regime == "tiny":
                    assert float(adv.abs().max()) < 2e-3
                if regime == "const":
                    assert float(adv.std()) == 0.0 and float(adv.mean()) == 0.75
                    assert float(R.reference(x, h, 1, 1)["g_newlogp"].abs().max()) == 0.0       # normalised advantage exactly 0
                if regime == "wide" and M >= 1025:
                    lo, hi_ = float((lr.exp() < 1 - h["clip"]).double().mean()), float((lr.exp() > 1 + h["clip"]).double().mean())
                    assert 0.25 < lo < 0.42 and 0.25 < hi_ < 0.42, (lo, hi_)
                if regime == "vclip" and M >= 1025:
                    assert 0.4 < float((dv.abs() > h["clip"]).double().mean()) < 0.6


def _draws():
    for M in M_TINY + M_CLASSES:
        for regime in R.REGIMES:
            for hi in range(len(R.HYPERS)):
                yield M, regime, hi
    for M in M_LARGE:
        for i, regime in enumerate(R.REGIMES):
            yield M, regime, i % len(R.HYPERS)
    for M in M_HUGE:
        yield M, "normal", 0


def test_margins_come_from_the_replay():
    """``replay`` (loss.hip's operation order in numpy float32, expf correctly rounded and then moved one ulp) against the CPU's Y, every
    (norm_adv, value mode) of every draw.  A class margin is the smallest power of two that covers twice the worst draw; the scalars at
    M >= TINY_M fit ref64.MARGIN_SCALARS.  Nothing here comes from the GPU kernels."""
    worst, where, count = collections.defaultdict(float), {}, 0
    for M, regime, hi in _draws():
        x = R.build_inputs(M, regime, hi)
        for na, vm in R.COMBOS:
            ref = R.reference(x, R.HYPERS[hi], na, vm)
            Y = R.yardstick(x, R.HYPERS[hi], na, vm, ref)
            for perturb in (False, True):
                _am, _sm, r = R.ratios(R.replay(x, R.HYPERS[hi], na, vm, perturb), ref, Y)
                for q, v in r.items():
                    key = (q, M >= R.TINY_M)
                    if v > worst[key]:
                        worst[key], where[key] = v, f"M{M}-{regime}-h{hi}-{'norm' if na else 'raw'}-v{vm}-{'ulp' if perturb else 'rounded'}"
            count += 1
    assert count >= 300
    print(f"\nreplay against the CPU yardstick over {count} draws (x 2 expf passes), worst ratio per class:")
    for (q, big), v in sorted(worst.items()):
        m = (R.MARGIN_SCALARS if big else R.MARGIN_SCALARS_TINY_M) if q == "scalars" else R.margin(q, R.TINY_M if big else 1)
        print(f"  {q:10s} {'M >= TINY_M' if big else 'M <  TINY_M'} {v:6.2f} x Y  (margin {m:g})  at {where[(q, big)]}")
        assert 2.0 * v <= m, (q, big, v, m, where[(q, big)])


# variant -> (the regime in which it is a different computation and must be rejected, in words; the same as a predicate on a draw)
_Draw = collections.namedtuple("_Draw", "M regime hi na vm")
EXPOSED_IN = collections.OrderedDict([
    ("std_over_M", ("norm_adv, 2 <= M <= 1025, every regime but 'const' (an = 0) and 'offset' (Y carries the mean's rounding)",
                    lambda d: d.na and 2 <= d.M <= 1025 and d.regime not in ("const", "offset"))),
    ("stats_fp32", ("regime 'offset' with norm_adv, M >= 1024", lambda d: d.regime == "offset" and d.na and d.M >= 1024)),
    ("vl_no_half", ("everywhere", lambda d: True)),
    ("g_newv_no_vf_coef", ("vf_coef != 1 (sets 0 and 2)", lambda d: d.hi != 1)),
    ("g_entropy_no_invM", ("ent_coef != 0 (sets 0 and 2), M > 1", lambda d: d.hi != 1 and d.M > 1)),
    ("g_entropy_wrong_sign", ("ent_coef != 0 (sets 0 and 2)", lambda d: d.hi != 1)),
    ("kl_swapped", ("everywhere", lambda d: True)),
    ("vmode_0_2_swapped", ("value modes 0 and 2", lambda d: d.vm != 1)),
    ("packed_ret_oldv_swapped", ("everywhere", lambda d: True)),
    ("last_block_dropped", ("M not a multiple of 1024, M <= 4097", lambda d: d.M % 1024 != 0 and d.M <= 4097)),
    ("stash_missing", ("everywhere", lambda d: True)),
    ("loss_no_entropy", ("ent_coef != 0 (sets 0 and 2)", lambda d: d.hi != 1)),
])
_VARIANT_DRAWS = []


def _variant_draws():
    if not _VARIANT_DRAWS:
        for M in (3, 65, 1024, 1025, 4097):
            for regime in R.REGIMES:
                for hi in range(len(R.HYPERS)):
                    x = R.build_inputs(M, regime, hi)
                    for na, vm in R.COMBOS:
                        ref = R.reference(x, R.HYPERS[hi], na, vm)
                        _VARIANT_DRAWS.append((_Draw(M, regime, hi, na, vm), x, ref, R.yardstick(x, R.HYPERS[hi], na, vm, ref)))
    return _VARIANT_DRAWS


def _over_bar(got, ref, Y, M):
    """The worst metric / (margin * Y) of a result over its classes; inf if it breaks the NaN / finiteness rules."""
    try:
        _am, _sm, r = R.ratios(got, ref, Y)
    except AssertionError:
        return float("inf")
    return max(v / (R.scalar_margin(M) if q == "scalars" else R.margin(q, M)) for q, v in r.items())


def test_the_correct_replay_passes_every_variant_draw():
    for d, x, ref, Y in _variant_draws():
        for perturb in (False, True):
            assert _over_bar(R.replay(x, R.HYPERS[d.hi], d.na, d.vm, perturb), ref, Y, d.M) <= 1.0, d


@pytest.mark.parametrize("variant", list(EXPOSED_IN))
def test_the_bars_reject_a_wrong_variant(variant):
    """Each wrong variant of ``replay`` must exceed its bar in EVERY draw of the regime that exposes it (M in {3, 65, 1024, 1025, 4097}, six
    regimes, three hyperparameter sets, six (norm_adv, value mode): 540 draws)."""
    assert set(EXPOSED_IN) == set(R.VARIANTS)
    words, exposed = EXPOSED_IN[variant]
    n_in = n_out = rej_out = 0
    lowest, missed = float("inf"), []
    for d, x, ref, Y in _variant_draws():
        over = _over_bar(R.replay(x, R.HYPERS[d.hi], d.na, d.vm, False, variant), ref, Y, d.M)
        if exposed(d):
            n_in += 1
            lowest = min(lowest, over)
            if not over > 1.0:
                missed.append((d, over))
        else:
            n_out += 1
            rej_out += over > 1.0
    print(f"\n{variant} ({R.VARIANTS[variant]}): exposed in [{words}], {n_in} draws, lowest metric / (margin * Y) {lowest:.3g}; "
          f"outside the regime {rej_out} of {n_out} draws rejected")
    assert n_in > 0 and not missed, (variant, len(missed), missed[:3])
