"""GPU: the layered PPO step and the layered rollout step at action heads of 17 .. 32 outputs (Humanoid's 17, the dexterous hands' 20 - 30,
a Categorical head of up to 32 choices: ``mlp_layered_layout(..., wide_actions=True)``, the library's ``wa`` entries, K13 / K14's builds
with 32-long per-action arrays), against the fp64 reference of tests/ref64.py used as it is.

T1  the step (``mlp_layered_step_native``), every case of tests/layered_actions_cases.py: the body of
    tests/test_layered_hidden_fp64_gpu.py::test_layered_step_matches_fp64_at_a_ragged_hidden_width -- reference, metric, GPU yardstick and
    the bars MARGIN / MARGIN_TINY_M / MARGIN_SCALARS unchanged; NaN-filled slack behind ``n_params`` stays untouched; a second launch gives
    the same bits.
T2  K13 alone (``head_ppo``): gz written over h equals gz written to a buffer of its own, bit for bit, and the last layers' bias
    gradients are the column sums of gz (tolerance of tests/test_layered_fp64_gpu.py).
T3  at 16 actions or fewer the ``wa`` entries are the entries that were there: scalars, gradients, gz, K14's actions, log-prob and value,
    bit for bit.
T4  K14 (``mlp_layered_act`` unpaired and paired, and ``head_act`` alone) at 17 and 32 actions against ``R.act_reference`` at MARGIN,
    ``R.safe_uniform`` draws for the Categorical head; guarded outputs; the value alone; and K14's stored action and log-prob fed back
    through K13 give old_kl == 0 and clipfrac == 0 exactly.
tests/test_layered_actions_host.py shows on the CPU that a correct fp32 computation meets T1's bars at every case's shape."""
import pytest
import torch

from tests import layered_act_cases as LA
from tests import layered_actions_cases as LW
from tests import ref64 as R
from tests import test_layered_ragged_fp64_gpu as LRG

pytestmark = pytest.mark.gpu

_Guarded = LRG._Guarded


def _policy(hidden, layers, D, A, cont, sd=None, seed=0):
    """The project's actor_critic on the GPU (the case's weights, or seeded ones moved off their initialisation), its flat bucket and
    its layered layout, taken with every keyword on."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(D, (A,) if cont else A, hidden, layers, 0.0, cont)
    if sd is not None:
        pol.load_state_dict(sd)
    pol = pol.cuda()
    if sd is None:
        with torch.no_grad():
            for p in pol.parameters():
                p.add_(0.05 * torch.randn_like(p))
    bucket = FlatBucket(pol.parameters())
    assert H.mlp_layout(pol, bucket) is None
    lay = H.mlp_layered_layout(pol, bucket, any_state=True, any_hidden=True, wide_actions=True)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (D, A, hidden, layers)
    assert bool(lay.get("wide_actions")) == (A > 16) and bool(lay.get("ragged_hidden")) == (hidden % 32 != 0)
    if sd is not None:
        assert [n for n, _ in pol.named_parameters()] == R.param_names(R.make_net(sd)), "FlatBucket order"
    return H, pol, bucket, lay


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))          # (adv_std of a one-sample minibatch is NaN)


def _step(H, obs, act, rec, idx, bucket, lay, c):
    g = torch.full((bucket.flat_grad.numel() + 64,), float("nan"), device="cuda")
    sc = H.mlp_layered_step_native(obs, act, rec, idx, bucket.flat_param, lay, g, R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"],
                                   c.norm_adv, c.vmode)
    torch.cuda.synchronize()
    return sc.clone(), g


# ---------------------------------------------------------------------------------- T1: the step
@pytest.mark.parametrize("c", LW.STEP_CASES, ids=LW.STEP_IDS)
def test_layered_step_matches_fp64_at_a_wide_action_head(c):
    data = R.build_case(c)
    ref = R.reference_step(c, data)
    data["ref"] = ref
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    H, _pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    assert lay["wide_actions"] is True
    obs, act, rec, idx = R.gpu_inputs(c, data)
    n = lay["n_params"]
    p0 = bucket.flat_param.clone()
    (sc, g), (sc2, g2) = _step(H, obs, act, rec, idx, bucket, lay, c), _step(H, obs, act, rec, idx, bucket, lay, c)
    assert bool(torch.isnan(g[n:]).all()), "the step wrote past n_params"
    assert not bool(torch.isnan(g[:n]).any()), "an entry of the gradient was not written"
    assert torch.equal(bucket.flat_param, p0), "the step wrote into the parameters"
    assert torch.equal(g[:n], g2[:n]) and _same(sc, sc2), "two launches differ"
    R.check_step(c, sc, g[:n], ref, Y, Ys, "layered, wide action head: aurppo_mlp_layered_wa_step_f32")


# ---------------------------------------------------------------------------------- T2: K13 alone
def _head_inputs(H, pol, lay, M, g):
    """Random last activations, actions, records close to the policy's own log-prob and value (every sample sends a gradient to both
    nets), and a permutation slice."""
    Hd, A, cont, L = lay["hidden"], lay["A"], lay["continuous"], lay["num_layers"]
    B = M + 37
    hA = torch.tanh(torch.randn(M, Hd, device="cuda", generator=g))
    hC = torch.tanh(torch.randn(M, Hd, device="cuda", generator=g))
    act = torch.randn(B, A, device="cuda", generator=g) if cont else torch.randint(0, A, (B,), device="cuda", generator=g).float()
    rec = torch.stack([-3 + 0.2 * torch.randn(B, device="cuda", generator=g), 2 * torch.randn(B, device="cuda", generator=g),
                       torch.randn(B, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)], 1).contiguous()
    idx = torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    with torch.no_grad():
        li = idx.long()
        out = pol.actor.net[2 * L](hA)
        if cont:
            ls = pol.actor_logstd.expand_as(out)
            lp = (-((act[li] - out) ** 2) / (2 * torch.exp(ls) ** 2) - ls - 0.9189385332046727).sum(1)
        else:
            lp = torch.log_softmax(out, 1).gather(1, act[li].long()[:, None])[:, 0]
        v = pol.critic.net[2 * L](hC).view(-1)
        rec[li, 0] = lp + 0.05 * torch.randn(M, device="cuda", generator=g)
        rec[li, 2] = v + torch.randn(M, device="cuda", generator=g)
        rec[li, 3] = v + 0.05 * torch.randn(M, device="cuda", generator=g)
    return hA, hC, act, rec, idx


def _head_layout_of(H, pol, bucket, Hd, D, A, cont, wide):
    seq, n, _D, _A, _cont, NL, _Hd = H._mlp_structure(pol, bucket, H.MLP_LAYERED_MAX_A)
    lay = dict(offsets=seq, n_params=n, D=D, A=A, continuous=cont, hidden=Hd, num_layers=NL, layered=True)
    if wide:
        lay["wide_actions"] = True
    return lay


def _head_ppo_both_ways(H, bucket, lay, hA, hC, act, rec, idx, M):
    outs = []
    for in_place in (False, True):
        a, cc = hA.clone(), hC.clone()
        ga, gc = (a, cc) if in_place else (torch.empty_like(a), torch.empty_like(cc))
        grad = torch.full_like(bucket.flat_grad, float("nan"))
        sc = H.head_ppo(a, cc, act, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, M > 1, H.VLOSS_CLIPPED, gzA=ga, gzC=gc)
        torch.cuda.synchronize()
        if not in_place:
            assert torch.equal(a, hA) and torch.equal(cc, hC), "the activations are inputs"
        outs.append((ga.clone(), gc.clone(), torch.nan_to_num(grad, nan=-7.0), torch.nan_to_num(sc, nan=-7.0)))
    return outs


@pytest.mark.parametrize("A,cont", [(17, True), (32, True), (32, False)], ids=["gauss17", "gauss32", "cat32"])
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("Hd", [32, 96, 1024])
def test_head_kernel_in_place_equals_separate_output_at_a_wide_action_head(Hd, M, A, cont):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    D = 16
    torch.manual_seed(Hd + M + A)
    pol = actor_critic(D, (A,) if cont else A, Hd, 1, 0.0, cont).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    bucket = FlatBucket(pol.parameters())
    lay = _head_layout_of(H, pol, bucket, Hd, D, A, cont, True)
    g = torch.Generator(device="cuda").manual_seed(Hd * 3 + M + A)
    hA, hC, act, rec, idx = _head_inputs(H, pol, lay, M, g)
    outs = _head_ppo_both_ways(H, bucket, lay, hA, hC, act, rec, idx, M)
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    ga, gc, grad, sc = outs[0]
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gc).all()) and float(ga.abs().max()) > 0 and float(gc.abs().max()) > 0
    hl, seq = H.head_layout(lay), lay["offsets"]
    # written: the heads (all A rows), actor_logstd and the two last-layer biases; the first layer's weights are not K13's
    assert bool((grad[hl[0]:hl[0] + A * Hd] != -7.0).all()) and bool((grad[hl[1]:hl[1] + A] != -7.0).all())
    assert bool((grad[hl[5]:hl[5] + Hd] != -7.0).all()) and bool((grad[hl[3]:hl[3] + 1] != -7.0).all())
    if cont:
        assert bool((grad[hl[4]:hl[4] + A] != -7.0).all())
    assert bool((grad[seq[0]:seq[0] + Hd * D] == -7.0).all())
    # the last hidden layer's bias gradient is the column sum of gz; the head's bias gradient belongs to the same sums
    torch.testing.assert_close(grad[hl[5]:hl[5] + Hd], ga.sum(0), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(grad[hl[6]:hl[6] + Hd], gc.sum(0), rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------- T3: 16 actions or fewer
@pytest.mark.parametrize("hidden,layers,D,A,cont", [(256, 2, 64, 16, True), (160, 1, 144, 5, False)], ids=["2x256-gauss16", "1x160-cat5"])
def test_at_16_actions_or_fewer_the_wa_entries_are_the_entries_that_were_there(hidden, layers, D, A, cont, monkeypatch):
    c = R._mk("layered", hidden, layers, D, A, cont, 257, True, 1)
    data = R.build_case(c)
    H, pol, bucket, lay = _policy(hidden, layers, D, A, cont, data["sd"])
    assert "wide_actions" not in lay
    forced = dict(lay, wide_actions=True)               # the wrappers then call the library's wa entries with A <= 16
    called = []
    check = H._check
    monkeypatch.setattr(H, "_check", lambda rc, name: (called.append(name), check(rc, name))[1])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    n = lay["n_params"]
    sc, g = _step(H, obs, act, rec, idx, bucket, lay, c)
    sc_w, g_w = _step(H, obs, act, rec, idx, bucket, forced, c)
    assert _same(sc, sc_w) and torch.equal(g[:n], g_w[:n]) and bool(torch.isnan(g_w[n:]).all())
    # K13 alone: gz, the gradients it writes, the scalars
    gen = torch.Generator(device="cuda").manual_seed(hidden + A)
    hA, hC, acts, recs, idxs = _head_inputs(H, pol, lay, 257, gen)
    old, new = _head_ppo_both_ways(H, bucket, lay, hA, hC, acts, recs, idxs, 257)[0], _head_ppo_both_ways(H, bucket, forced, hA, hC, acts, recs, idxs, 257)[0]
    for name, x, y in zip(("gzA", "gzC", "gradients", "scalars"), old, new):
        assert torch.equal(x, y), f"K13: {name} differs through the wa entry"
    # K14 alone and the rollout step
    N = obs.shape[0]
    noise = torch.randn(N, A, device="cuda", generator=gen) if cont else torch.rand(N, device="cuda", generator=gen)
    hA, hC = torch.tanh(torch.randn(N, hidden, device="cuda", generator=gen)), torch.tanh(torch.randn(N, hidden, device="cuda", generator=gen))
    for x, y in zip(H.head_act(hA, hC, noise, bucket.flat_param, lay), H.head_act(hA, hC, noise, bucket.flat_param, forced)):
        assert torch.equal(x, y), "K14 differs through the wa entry"
    for kw in ({}, dict(paired=True)):
        out = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, **kw)
        out_w = H.mlp_layered_act(obs, noise, bucket.flat_param, forced, **kw)
        torch.cuda.synchronize()
        for x, y in zip(out, out_w):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y), f"the rollout step differs through the wa entry ({kw})"
    assert [e for e in called if "_wa_" in e] == ["aurppo_mlp_layered_wa_step_f32", "aurppo_head_ppo_wa_f32", "aurppo_head_ppo_wa_f32",
                                                  "aurppo_head_act_wa_f32", "aurppo_mlp_layered_wa_act_f32", "aurppo_mlp_layered_wa_act_paired_f32"]
    lib = H._lib_or_raise()
    assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(257, D, A, hidden, layers) == lib.aurppo_mlp_layered_step_workspace_bytes(257, D, A, hidden, layers) > 0
    assert lib.aurppo_head_ppo_wa_workspace_bytes(257, hidden, A) == lib.aurppo_head_ppo_workspace_bytes(257, hidden, A) > 0


# ---------------------------------------------------------------------------------- T4: K14
_ACT_SHAPES = {(17, True): (256, 2, 64, "normal"), (32, True): (1024, 1, 144, "bf16half"), (17, False): (96, 1, 144, "normal"),
               (32, False): (160, 2, 64, "normal")}


@pytest.mark.parametrize("N", [1, 257, 2049])
@pytest.mark.parametrize("A,cont", sorted(_ACT_SHAPES), ids=[f"{'gauss' if cont else 'cat'}{A}" for A, cont in sorted(_ACT_SHAPES)])
def test_layered_act_and_head_act_match_fp64_at_a_wide_action_head(A, cont, N):
    hidden, layers, D, regime = _ACT_SHAPES[(A, cont)]
    c = R._mk("layered", hidden, layers, D, A, cont, N, False, 0, regime)
    data = LA.build(c)
    ref = data["ref"]
    Y, _y = LA.yardstick(c, data, "cuda")
    H, pol, bucket, lay = _policy(hidden, layers, D, A, cont, data["sd"])
    assert lay["wide_actions"] is True
    obs, noise = data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous()
    p0 = bucket.flat_param.clone()

    def guarded(call):
        ga, gl, gv = _Guarded(*((N, A) if cont else (N,))), _Guarded(N), _Guarded(N)
        a, lp, v = call(ga.view, gl.view, gv.view)
        torch.cuda.synchronize()
        assert a is ga.view and lp is gl.view and v is gv.view
        assert ga.guards_intact() and gl.guards_intact() and gv.guards_intact(), "a guard was written"
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(v).all())
        return a.clone(), lp.clone(), v.clone()

    def held(label, a, lp, v):
        if not cont:
            assert torch.equal(a.long().cpu(), ref["action"]), (label, int((a.long().cpu() != ref["action"]).sum()))
        m = LA.metrics(c, ref, v, a, lp)
        print(f"\n[{label}] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items())
              + f" (Y {Y:.3e}; moved {data['moved']})")
        for n, x in m.items():
            assert x <= R.MARGIN * Y, (label, n, x, Y, x / Y)

    a, lp, v = guarded(lambda *out: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, *out))
    held("layered act: aurppo_mlp_layered_wa_act_f32", a, lp, v)
    for got, first in zip(guarded(lambda *out: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, *out, paired=True)), (a, lp, v)):
        assert torch.equal(got, first), "the paired step differs from the unpaired one"
    for kw in ({}, dict(paired=True)):
        gv = _Guarded(N)
        a0, lp0, v0 = H.mlp_layered_act(obs, None, bucket.flat_param, lay, value=gv.view, **kw)
        torch.cuda.synchronize()
        assert a0 is None and lp0 is None and torch.equal(v0, v) and gv.guards_intact()
    # K14 alone, on the last activations as the library's own product leaves them
    hs = []
    for net in (pol.actor.net, pol.critic.net):
        h = obs
        for l in range(layers):
            h = H.linear_bias_act(h, net[2 * l].weight.detach(), net[2 * l].bias.detach(), act=1)
        hs.append(h.contiguous())
    hA, hC = hs
    ka, klp, kv = guarded(lambda *out: H.head_act(hA, hC, noise, bucket.flat_param, lay, *out))
    held("K14 alone: aurppo_head_act_wa_f32", ka, klp, kv)
    gv = _Guarded(N)
    a0, lp0, v0 = H.head_act(None, hC, None, bucket.flat_param, lay, value=gv.view)
    torch.cuda.synchronize()
    assert a0 is None and lp0 is None and torch.equal(v0, kv) and gv.guards_intact()
    # K14's stored action and log-prob back through K13 at the same parameters: the ratio is exp(0) for every row
    g = torch.Generator(device="cuda").manual_seed(N + A)
    rec = torch.stack([klp, torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g), kv], 1).contiguous()
    idx = torch.randperm(N, device="cuda", generator=g).to(torch.int32).contiguous()
    grad = torch.full_like(bucket.flat_grad, float("nan"))
    li = idx.long()                                 # K13's activations are in minibatch order: row r belongs to sample idx[r]
    sc = H.head_ppo(hA[li].contiguous(), hC[li].contiguous(), ka.contiguous(), rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, N > 1, H.VLOSS_CLIPPED).cpu()
    print(f"K13 on K14's rows: old_kl {float(sc[H.S_OLD_KL])!r}, kl {float(sc[H.S_KL])!r}, clipfrac {float(sc[H.S_CLIPFRAC])!r}")
    assert float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0
    assert torch.equal(bucket.flat_param, p0)
