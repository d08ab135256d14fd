"""CPU: the layered routes at state widths that are no multiple of 16 (tests/layered_ragged_cases.py).  (1) For every case of the GPU
test, ANOTHER correct fp32 computation -- ``ref64.make_alternative_fp32_net`` -- meets the same bars against the CPU yardstick, for the
step and for the rollout step (the bodies of tests/test_layered_host.py and tests/test_layered_act_host.py): the bars the GPU test holds
the kernels to can be met at these shapes without exclusions.  (2) Which policies ``hip_ops.mlp_layered_layout`` takes with
``any_state=True`` and which it still refuses (it needs no device).  (3) What ``mlp_layered_step``, ``mlp_layered_prepare`` and
``mlp_layered_act`` hand to the library at D = 17 equals tests/transcripts/layered_ragged_calls.json (the recorder of
tests/test_hip_ops_calls.py, imported): the same calls in the same order as at D = 16, no new argument.

Re-record with ``python tests/test_layered_ragged_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import layered_act_cases as LA              # noqa: E402
from tests import layered_ragged_cases as LR           # noqa: E402
from tests import ref64 as R                           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_ragged_calls.json")
N, A, D, HIDDEN = 4, TC.A, 17, 160


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)       # fixed summation order in the CPU yardstick
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------ (1) the bars can be met at these shapes
@pytest.mark.parametrize("c", LR.STEP_CASES, ids=LR.STEP_IDS)
def test_a_second_correct_fp32_formulation_meets_the_bars_at_the_ragged_step_shapes(c, one_thread):
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cpu")
    li = data["idx"].long()
    got = R.run_step(R.make_alternative_fp32_net(data["sd"]), data["obs"][li], data["act"][li] if c.cont else data["act"][li].long(),
                     data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    R.check_step(c, got["scalars"], got["flat"], data["ref"], Y, Ys, "alternative fp32")


@pytest.mark.parametrize("c", LR.ACT_CASES, ids=LR.ACT_IDS)
def test_a_second_correct_fp32_formulation_meets_the_bar_at_the_ragged_act_shapes(c, one_thread):
    data = LA.build(c)
    Y, y = LA.yardstick(c, data, "cpu")
    alt = R.make_alternative_fp32_net(data["sd"])
    m = LA.metrics(c, data["ref"], *LA.torch_fp32_step(c, data, "cpu", net=alt))
    print(f"\n[alternative fp32] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items()) + f" (Y {Y:.3e})")
    for n, x in m.items():
        assert x <= R.MARGIN * Y, (n, x, Y, x / Y)
    if not c.cont:
        # the second formulation samples the reference's index too: its CDF, as K14 forms it, against the safe draws
        with torch.no_grad():
            mu = alt.actor(data["obs"])
            lse = mu.max(1, keepdim=True).values + torch.log(torch.exp(mu - mu.max(1, keepdim=True).values).sum(1, keepdim=True))
            cdf = torch.exp(mu - lse).cumsum(1)
        pick = (data["noise"][:, None] >= cdf[:, :-1]).sum(1)
        assert torch.equal(pick, data["ref"]["action"])


# ------------------------------------------------------------------ (2) the layout rule
def _layouts(hidden, layers, D_, A_, cont=True, **kw):
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(D_, (A_,) if cont else A_, hidden, layers, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    return H.mlp_layout(pol, bucket), H.mlp_layered_layout(pol, bucket, **kw)


@pytest.mark.parametrize("hidden,layers,D_,A_", [(256, 2, 17, 6), (64, 1, 376, 16), (256, 2, 20, 6)])
def test_any_state_gives_a_ragged_policy_a_layered_layout(hidden, layers, D_, A_):
    fused, lay = _layouts(hidden, layers, D_, A_, any_state=True)
    assert fused is None and isinstance(lay, dict) and lay["layered"] is True
    assert (lay["hidden"], lay["num_layers"], lay["D"], lay["A"], lay["continuous"]) == (hidden, layers, D_, A_, True)
    assert len(lay["offsets"]) == 4 * (layers + 1) + 1 and len(H.head_layout(lay)) == 7
    n_w = sum((D_ * hidden + hidden) + (layers - 1) * (hidden * hidden + hidden) + (out * hidden + out) for out in (A_, 1))
    assert lay["n_params"] == n_w + A_


@pytest.mark.parametrize("hidden,layers,D_,A_", [(100, 2, 17, 6), (256, 2, 17, 17), (1056, 2, 17, 6)])
def test_any_state_drops_the_state_condition_only(hidden, layers, D_, A_):
    """A hidden width off 32 (K7w's if it is narrow enough), 17 actions, a hidden width past 1024: no layered layout either way."""
    _fused, layered = _layouts(hidden, layers, D_, A_, any_state=True)
    assert layered is None and _layouts(hidden, layers, D_, A_)[1] is None


@pytest.mark.parametrize("hidden,layers,D_,A_", [(64, 2, 17, 6), (128, 3, 11, 6), (64, 2, 64, 6), (128, 3, 128, 6)])
def test_the_fused_kernels_shapes_stay_with_them_under_any_state(hidden, layers, D_, A_):
    fused, layered = _layouts(hidden, layers, D_, A_, any_state=True)
    assert fused is not None and layered is None


def test_without_the_keyword_a_ragged_state_is_still_refused():
    assert _layouts(256, 2, 20, 6) == (None, None)
    assert _layouts(256, 2, 20, 6, any_state=False) == (None, None)
    assert _layouts(256, 2, 17, 6) == (None, None)


@pytest.mark.parametrize("c", LR.STEP_CASES + LR.ACT_CASES, ids=["step-" + i for i in LR.STEP_IDS] + ["act-" + i for i in LR.ACT_IDS])
def test_every_case_is_a_ragged_layered_shape(c):
    fused, lay = _layouts(c.hidden, c.layers, c.D, c.A, c.cont, any_state=True)
    assert fused is None and lay is not None
    if c.D % 16:
        assert _layouts(c.hidden, c.layers, c.D, c.A, c.cont)[1] is None


# ------------------------------------------------------------------ (3) what the host layer hands to the library at D = 17
CASES = {}
M, B = TC.M, TC.B


def _ragged(h, layers, cont, packed):
    """(layout, bucket, obs, actions, rec, idx) of a ``layers`` x 160 policy over a state of 17 floats, its layout through ``any_state``."""
    pol, bucket = TC._policy(h, D, HIDDEN, layers, cont)
    assert H.mlp_layered_layout(pol, bucket) is None
    lay = H.mlp_layered_layout(pol, bucket, any_state=True)
    assert lay["D"] == D and lay["hidden"] == HIDDEN and lay["offsets"][2] != 0 and lay["continuous"] == cont
    obs = h.t("obs", B, D)
    if packed:
        actions, rec = None, h.t("rec64", B, 16)
    else:
        actions, rec = (h.t("actions", B, A) if cont else h.t("actions", B)), h.t("rec", B, 4)
    return lay, bucket, obs, actions, rec, h.idx("idx")


def _step_case(layers, cont, packed):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _ragged(h, layers, cont, packed)
        H._layered_cache.clear()
        sc = h.t("scalars", 9)
        assert H.mlp_layered_step(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True,
                                  H.VLOSS_OLDVALUES, sc) is sc
        for net, acts in enumerate(H._layered_buffers(M, lay, obs.device)):
            for l, a in enumerate(acts):
                h.name(f"act{net}.{l}", a)
        H._layered_cache.clear()
    return run


def _outs(h, cont):
    return (h.t("actions_out", N, A) if cont else h.t("actions_out", N)), h.t("logp", N), h.t("value", N)


def _act_case(layers, cont, mode):
    def run(h):
        lay, bucket, *_ = _ragged(h, layers, cont, False)
        obs = h.t("obs4", N, D)
        if mode == "value_only":
            a, lp, v = H.mlp_layered_act(obs, None, bucket.flat_param, lay)
            assert a is None and lp is None and v.shape == (N,)
            h.name("value_new", v)
            H.mlp_layered_act(obs, None, bucket.flat_param, lay, value=h.t("value", N))
        else:
            nz = h.t("noise", N, A) if cont else h.t("noise", N)
            wop = H.mlp_layered_prepare(bucket.flat_param, lay)
            assert H.mlp_layered_prepare(bucket.flat_param, lay) is wop
            assert H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont), wop=wop)[0].shape == ((N, A) if cont else (N,))
            H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont))
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
    return run


CASES["mlp_layered_step/D17/L1/continuous/packed"] = _step_case(1, True, True)
CASES["mlp_layered_step/D17/L3/categorical"] = _step_case(3, False, False)
CASES["mlp_layered_act/D17/L1/continuous/prepared"] = _act_case(1, True, "prepared")
CASES["mlp_layered_act/D17/L3/categorical/value_only"] = _act_case(3, False, "value_only")


def run_case(name, setattr_, bound=None):
    h = TC.Harness(bound)
    h.install(setattr_)
    setattr_(torch.cuda, "current_device", lambda: 0)
    H._layered_wop_cache.clear()
    try:
        CASES[name](h)
        return json.loads(json.dumps(h.transcript()))
    finally:
        H._layered_wop_cache.clear()


def _recorded():
    with open(TRANSCRIPT) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(_recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_match_the_recorded_transcript(name, monkeypatch):
    got, want = run_case(name, monkeypatch.setattr), _recorded()[name]
    assert len(got) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs"
    assert len(got) == len(want)


def test_the_state_width_reaches_the_library_as_it_is(monkeypatch):
    """Layer 0's three products, the prepare call and the act call carry 17, not a padded width; the shared workspace is sized from it."""
    rec = _recorded()
    step = rec["mlp_layered_step/D17/L3/categorical"]
    by_fn = {}
    for fn, args in step:
        by_fn.setdefault(fn, []).append(args)
    assert all(a[6] == D and a[7] == HIDDEN for a in by_fn["aurppo_linear_rows_bias_act_f32"]) and len(by_fn["aurppo_linear_rows_bias_act_f32"]) == 2
    assert all(a[5] == HIDDEN and a[6] == D for a in by_fn["aurppo_linear_wgrad_rows_f32"]) and len(by_fn["aurppo_linear_wgrad_rows_f32"]) == 2
    assert by_fn["aurppo_conv3x3_wop_bytes"] == [[HIDDEN, HIDDEN]]      # max(D, hidden), hidden
    act = rec["mlp_layered_act/D17/L1/continuous/prepared"]
    assert all(args[3] == D for fn, args in act if fn == "aurppo_mlp_layered_prep_f32")
    assert all(args[3] == D for fn, args in act if fn == "aurppo_mlp_layered_act_f32")
    assert all(args[0] == D for fn, args in act if fn == "aurppo_mlp_layered_wop_bytes")


def test_every_call_fits_the_bound_argtypes(monkeypatch):
    """The same cases against the real binding's ``argtypes`` (count and ctypes conversion; nothing is launched)."""
    import __graft_entry__ as g
    g.build()
    bound = TC._lib.load()
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


def test_the_size_functions_round_a_ragged_inner_dimension_up():
    """Whole k-steps of 16 columns: the sizes at K = 17 .. 32 are the size at 32, multiples of 16 keep their values, and the shared
    "conv" workspace of a D = 376, hidden = 64 step holds layer 0's 24 k-steps (a floor would give 23)."""
    import __graft_entry__ as g
    g.build()
    lib = TC._lib.load()
    for K in (1, 11, 17, 31):
        up = (K + 15) // 16 * 16
        assert lib.aurppo_conv3x3_wop_bytes(K, 256) == lib.aurppo_conv3x3_wop_bytes(up, 256)
        assert lib.aurppo_mlp_layered_wop_bytes(K, 256, 2) == lib.aurppo_mlp_layered_wop_bytes(up, 256, 2) > 0
    assert lib.aurppo_conv3x3_wop_bytes(144, 160) == (5 + 4) * 9 * 9 * 3 * 1024 + 64
    assert lib.aurppo_mlp_layered_wop_bytes(64, 256, 2) == 2 * ((8 + 4) * 4 * 3 * 1024 + (8 + 4) * 16 * 3 * 1024)
    need = (2 + 4) * 24 * 3 * 1024          # k_linear_tail at N = 64 reads (2 blocks + one group of slack) x 24 k-steps x 3 planes
    assert lib.aurppo_conv3x3_wop_bytes(max(376, 64), 64) >= need
    assert lib.aurppo_mlp_layered_wop_bytes(376, 64, 1) == 2 * need
    assert lib.aurppo_mlp_layered_wop_bytes(0, 256, 2) == 0 and lib.aurppo_mlp_layered_wop_bytes(17, 100, 2) == 0


if __name__ == "__main__":
    class _Patch:
        def __init__(self):
            self.undo = []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

        def restore(self):
            for obj, name, old in reversed(self.undo):
                setattr(obj, name, old)

    result = {}
    for case_name in sorted(CASES):
        patch = _Patch()
        try:
            result[case_name] = run_case(case_name, patch.setattr)
        finally:
            patch.restore()
    os.makedirs(os.path.dirname(TRANSCRIPT), exist_ok=True)
    with open(TRANSCRIPT, "w") as f:
        f.write(TC._dump(result))
    print(f"{len(result)} cases, {sum(len(v) for v in result.values())} calls -> {TRANSCRIPT}")
