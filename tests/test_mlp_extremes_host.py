"""Host (no GPU): the regimes of tests/ref64_extremes.py are what they say, the band of tests/test_mlp_extremes_fp64_gpu.py is one a
correct fp32 computation meets, and it has teeth (DESIGN 2.6 has the figures these tests print with ``-s``)."""
import numpy as np
import pytest
import torch

from tests import ref64 as R
from tests import ref64_extremes as X


@pytest.fixture
def one_thread():
    """The yardstick is an fp32 matrix product on the CPU: one thread fixes its summation order."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("c", X.STEP_CASES, ids=R.case_id)
def test_step_cases_meet_their_regimes_condition_and_the_reference_is_finite(c):
    data = X.build_case(c)                 # asserts the condition and zero samples near a branch point
    print(f"\n{R.case_id(c)}: moved {data['moved']}; " + "; ".join(f"{k} {lo:.4g} .. {hi:.4g}" for k, (lo, hi) in data["cond"].items()))
    li = data["idx"].long()
    with torch.no_grad():
        _, lp, _, v = data["net64"].evaluate(data["obs"][li].double(), data["act"][li].double() if c.cont else data["act"][li].long())
    d = R.branch_distances(lp, v.reshape(-1), data["rec"][li], R.HYPER["clip"], c.norm_adv, c.vmode)
    assert all(float(x.min()) >= R.BRANCH_EPS for x in d.values()), {k: float(x.min()) for k, x in d.items()}
    if c.regime in ("tight", "loose"):     # the actions come from the policy: z stays O(1) at either sigma
        with torch.no_grad():
            z = (data["act"][li].double() - data["net64"].actor(data["obs"][li].double())) / data["net64"].actor_logstd.exp()
        assert 3.0 < float(z.abs().max()) < 6.0, float(z.abs().max())
    ref = R.reference_step(c, data)
    for k in ("scalars", "flat", "logp", "ent", "value", "scalar_scales"):
        assert bool(torch.isfinite(ref[k]).all()), k
    for n, S in zip(ref["names"], ref["grad_scales"]):
        assert bool(torch.isfinite(S).all()) and float(S.min()) > 0, n


@pytest.mark.parametrize("c", X.ACT_CASES, ids=R.case_id)
def test_rollout_cases_meet_their_regimes_condition(c):
    data = X.build_act(c)
    ref = data["ref"]
    print(f"\n{R.case_id(c)}: moved {data['moved']}; " + "; ".join(f"{k} {lo:.4g} .. {hi:.4g}" for k, (lo, hi) in data["cond"].items()))
    assert bool(torch.isfinite(ref["value"]).all()) and bool(torch.isfinite(ref["logp"]).all())
    if not c.cont:
        assert float((data["noise"].double()[:, None] - ref["cdf"][:, :-1]).abs().min()) >= R.BRANCH_EPS


def test_shapes_dispatch_to_the_families_the_cases_name():
    """Which family a shape belongs to, without a device: K7 / K7w by ``mlp_layout``, the layered route where it gives None."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    for c in {(c.kind, c.hidden, c.layers, c.D, c.A, c.cont): c for c in X.STEP_CASES + X.ACT_CASES}.values():
        pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
        bucket = FlatBucket(pol.parameters())
        lay = H.mlp_layout(pol, bucket)
        if c.kind == "layered":
            assert lay is None and H.mlp_layered_layout(pol, bucket) is not None, c
        else:
            assert lay is not None and lay["wide"] == (c.kind == "k7w"), c


# ------------------------------------------------------------------ the bars are what a correct computation can meet
_SHAPES = {"k7": ("k7", 64, 2, 16, 6), "k7w": ("k7w", 96, 2, 65, 6), "layered": ("layered", 160, 2, 64, 6)}
N_SEEDS = 8


@pytest.mark.parametrize("shape", list(_SHAPES))
@pytest.mark.parametrize("regime", X.REGIMES)
def test_a_second_rendition_meets_the_bars_against_the_band_without_it(regime, shape, one_thread):
    """F2 (exp2 and reciprocal-then-multiply: the kernels' own operation order) judged like a kernel against max(Y, F): every gradient
    tensor <= MARGIN, every scalar <= MARGIN_SCALARS, over N_SEEDS seeds at M 1000."""
    kind, hidden, layers, D, A = _SHAPES[shape]
    cont = regime != "peaked"
    worst_g = worst_s = 0.0
    for seed in range(N_SEEDS):
        c = X.mk(kind, hidden, layers, D, A, cont, regime, seed % 2 == 0, seed % 3)._replace(seed=7000 + 10 * seed + len(shape))
        data = X.build_case(c)
        data["ref"] = R.reference_step(c, data)
        band = X.band_step(c, data, "cpu", kinds=("F",))
        got = X.rendition_step(c, data, "F2")
        _, _, rg, rs = X.check_step_band(c, got["scalars"], got["flat"], data["ref"], band, f"F2 / max(Y, F), {shape}, seed {seed}")
        worst_g, worst_s = max(worst_g, rg), max(worst_s, rs)
    print(f"\nF2 against max(Y, F), {shape}, {regime}: worst gradient ratio {worst_g:.2f} (margin {R.MARGIN:g}), worst scalar ratio "
          f"{worst_s:.2f} (margin {R.MARGIN_SCALARS:g})")


@pytest.mark.parametrize("regime", X.CAT_REGIMES[:3])
def test_the_second_rendition_meets_the_bars_behind_a_categorical_head(regime, one_thread):
    worst_g = worst_s = 0.0
    for seed in range(N_SEEDS):
        c = X.mk("k7", 64, 2, 16, 6, False, regime, seed % 2 == 0, seed % 3)._replace(seed=9000 + seed)
        data = X.build_case(c)
        data["ref"] = R.reference_step(c, data)
        band = X.band_step(c, data, "cpu", kinds=("F",))
        got = X.rendition_step(c, data, "F2")
        _, _, rg, rs = X.check_step_band(c, got["scalars"], got["flat"], data["ref"], band, f"F2 / max(Y, F), categorical, seed {seed}")
        worst_g, worst_s = max(worst_g, rg), max(worst_s, rs)
    print(f"\nF2 against max(Y, F), k7 categorical, {regime}: worst gradient ratio {worst_g:.2f}, worst scalar ratio {worst_s:.2f}")


_ACT_SHAPES = [("k7", 64, 2, 16), ("k7w", 64, 1, 64), ("k7w", 128, 3, 128), ("layered", 160, 2, 64)]


@pytest.mark.parametrize("cont", [True, False], ids=["gauss", "cat"])
@pytest.mark.parametrize("kind,hidden,layers,D", _ACT_SHAPES, ids=[f"{k}-{l}x{h}-D{D}" for k, h, l, D in _ACT_SHAPES])
def test_the_rollout_steps_class_margin_in_deep_is_what_another_summation_order_needs(kind, hidden, layers, D, cont, one_thread):
    """The same fp32 products summed in two other orders (``ref64_extremes.make_order_net``), judged like K8 / K8w / K14 against the full
    band at N 257 in ``deep``: up to 2.66 x B over 384 draws (24 seeds; 8 here), i.e. over MARGIN and under MARGIN_ACT_DEEP."""
    from tests import layered_act_cases as LA
    worst = 0.0
    for seed in range(8):
        c = X.mk(kind, hidden, layers, D, 6, cont, "deep", False, 0, M=X.N_ACT)._replace(seed=500 + seed)
        data = X.build_act(c)
        band = X.band_act(c, data, "cpu")
        for order in ("rev", "four"):
            with torch.no_grad():
                m = X.act_metrics(c, data["ref"], *LA.torch_fp32_step(c, data, "cpu", net=X.make_order_net(data["sd"], order)))
            worst = max(worst, max(m.values()) / band["B"])
            assert max(m.values()) <= X.act_margin(c) * band["B"], (order, seed, m, band)
    print(f"\nrollout step in deep, {layers} x {hidden}, D {D}, {'Gaussian' if cont else 'Categorical'}: another summation order reaches {worst:.2f} x B "
          f"(MARGIN {R.MARGIN:g}, MARGIN_ACT_DEEP {X.MARGIN_ACT_DEEP:g})")


# ------------------------------------------------------------------ the bars have teeth
_TEETH = {}


def _teeth(regime):
    """A case of the GPU test in ``regime`` (Gaussian regimes: K7's 2 x 64, D 16, A 6; ``peaked``: K7w's 1 x 128, D 4, A 16, whose logits
    pass 89 and whose lowest log-prob is below -104, where e^x overflows and underflows in fp32 on any machine) with its reference and
    its FULL band on the CPU, built once."""
    if regime not in _TEETH:
        c, = [c for c in (X.K7W_WIDER_STEP if regime == "peaked" else X.K7_STEP) if c.regime == regime and c.cont == (regime != "peaked")]
        data = X.build_case(c)
        data["ref"] = R.reference_step(c, data)
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        band = X.band_step(c, data, "cpu")
        torch.set_num_threads(n)
        _TEETH[regime] = (c, data, band)
    return _TEETH[regime]


def _judge(regime, kind="F2", head="kernel", net=None):
    """(gradient ratio over B, scalar ratio over max Bs) of a mutant, or the AssertionError's text if an output is non-finite."""
    c, data, band = _teeth(regime)
    got = X.rendition_step(c, data, kind, head, net)
    try:
        gm, sm = R.grad_metrics(got["flat"], data["ref"]), R.scalar_metrics(got["scalars"], data["ref"])
    except AssertionError as e:
        return None, None, str(e)
    return max(gm.values()) / band["B"], max(sm.values()) / max(band["Bs"].values()), None


def test_the_band_itself():
    for regime in X.REGIMES:
        _c, _data, band = _teeth(regime)
        rg, rs, err = _judge(regime, "F2")
        print(f"\n{regime}: " + ", ".join(f"{k} {v:.3e}" for k, v in band["parts"].items()) + f"; F2 {rg:.2f} x B, scalars {rs:.2f} x Bs")
        assert err is None and rg <= R.MARGIN and rs <= R.MARGIN_SCALARS


def test_tanh_prime_from_autograd_of_the_formula_is_rejected_in_deep():
    rg, rs, err = _judge("deep", "autograd")
    assert err is not None and "non-finite gradient" in err, (rg, rs, err)
    rg, rs, err = _judge("saturated", "autograd")         # ... and is a correct computation short of the overflow
    assert err is None and rg <= R.MARGIN and rs <= R.MARGIN_SCALARS, (rg, rs, err)


def _peaked_logits():
    c, data, _band = _teeth("peaked")
    with torch.no_grad():
        return data["net64"].actor(data["obs"][data["idx"].long()].double())


def test_softmax_without_max_subtraction_is_rejected_in_peaked():
    assert float(_peaked_logits().max()) > 89.0                       # e^logit overflows in fp32
    rg, rs, err = _judge("peaked", "F2", "no_max")
    assert err is not None, (rg, rs)


def test_entropy_from_the_log_of_the_fp32_probability_is_rejected_in_peaked():
    assert float(torch.log_softmax(_peaked_logits(), 1).min()) < -104.0    # a probability that is 0 in fp32 even with denormals kept
    rg, rs, err = _judge("peaked", "F2", "log_p")
    assert err is not None, (rg, rs)


def test_an_exponential_good_to_twelve_bits_is_rejected():
    for regime in X.GAUSS_REGIMES:
        rg, rs, err = _judge(regime, "exp12")
        print(f"\nexp to 2^-12, {regime}: gradients {rg:.1f} x B, scalars {rs:.1f} x Bs (bars {R.MARGIN:g} / {R.MARGIN_SCALARS:g})")
        if regime in ("linear", "saturated", "tight"):
            assert err is None and rg > R.MARGIN, (regime, rg)


def test_a_tanh_above_one_is_rejected():
    """t + 2^-22 for every unit: 1 - t^2 turns negative where the unit is saturated.  Against the band that is a draw (0.85 - 5.6 x B
    over the regimes: printed per regime, asserted where the host run finds it over the bar); the check that rejects it whatever the
    case is the sweep's |y| <= 1."""
    x = X.tanh_sweep_points(1 << 16)
    for kind in ("F", "F2"):
        X.check_tanh_sweep(x, X._TanhFn.apply(x, kind, None), f"rendition {kind}")
    p = X._TanhFn.apply(x, "P", np.random.RandomState(0))      # the envelope: inside the bound and inside [-1, 1], not exact at |x| >= 10
    worst = float((p.double() - torch.tanh(x.double())).abs().max())
    print(f"rendition P: {worst / R.ULP32:.2f} units of 2^-24")
    assert worst <= X.TANH_BOUND and float(p.abs().max()) <= 1.0
    for kind in ("over1", "exp12"):
        with pytest.raises(AssertionError):
            X.check_tanh_sweep(x, X._TanhFn.apply(x, kind, None), f"mutant {kind}")
    seen = {}
    for regime in X.REGIMES:
        rg, rs, err = _judge(regime, "over1")
        seen[regime] = rg
        print(f"\n|t| above 1, {regime}: gradients {rg:.2f} x B, scalars {rs:.2f} x Bs")
    assert max(seen.values()) > R.MARGIN, seen
    for regime in OVER1_REJECTED_IN:
        assert seen[regime] > R.MARGIN, (regime, seen)


def test_missing_third_order_products_are_rejected_where_the_band_can_see_them():
    """All three third-order plane products missing from every role (``ref64.make_emulated_net``, torch's tanh).  Asserted in the regimes
    where the host run finds it at >= 1.5 x the bar; DESIGN 2.6 names the regimes that cannot see it."""
    seen = {}
    for regime in X.REGIMES:
        c, data, band = _teeth(regime)
        net = R.make_emulated_net(data["sd"], lambda l, r: R.SIX - set(R.THIRD_ORDER))
        rg, rs, err = _judge(regime, net=net)
        seen[regime] = rg
        print(f"\nthird order missing everywhere, {regime}: gradients {rg:.2f} x B (bar {R.MARGIN:g}), scalars {rs:.2f} x Bs")
    for regime in THIRD_ORDER_REJECTED_IN:
        assert seen[regime] > R.MARGIN, (regime, seen)
    assert all(seen[r] >= 1.5 * R.MARGIN for r in THIRD_ORDER_REJECTED_IN) and all(seen[r] < 1.5 * R.MARGIN for r in X.REGIMES if r not in THIRD_ORDER_REJECTED_IN), seen


OVER1_REJECTED_IN = ("loose",)
THIRD_ORDER_REJECTED_IN = ("saturated", "deep", "tight", "loose", "peaked")
