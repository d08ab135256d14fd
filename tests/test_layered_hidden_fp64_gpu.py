"""GPU: the layered PPO step and the layered rollout step at hidden widths that are no multiple of 32 (200, 300, 400, 500, 100 over
Humanoid's 376 state floats, ...: ``mlp_layered_layout(..., any_state=True, any_hidden=True)``, the library's ``anyh`` entries, which run
the policy at the width rounded up to 32 with zero planes for what the bucket does not have), against the fp64 reference of
tests/ref64.py used as it is, and against the zero-padded policy through the entries that were there before.

T1  the step (``mlp_layered_step_native``): the body of tests/test_layered_ragged_fp64_gpu.py::test_layered_step_matches_fp64_at_a_ragged_state
    -- reference, metric, GPU yardstick and the bars MARGIN / MARGIN_TINY_M / MARGIN_SCALARS unchanged; the gradient buffer is NaN-filled
    with 64 floats behind it: nothing past ``n_params`` is written, no NaN is left inside, ``flat_param`` is unchanged, a second launch
    gives the same bits.
T2  the rollout step, unpaired and paired: the body of test_layered_act_matches_fp64_at_a_ragged_state -- guarded, misaligned outputs, a
    repeat, prepared weights, value-only; bar MARGIN, every Categorical index equal; paired equals unpaired bit for bit.
T3  the design: the Hp-wide policy whose parameters are the ragged policy's with zeros elsewhere, through the EXISTING entries on its own
    aligned layout, gives the same bits -- nine scalars, every real gradient entry, actions, log-prob, value -- and exact zeros at its pad
    positions.  So the K13 / K14 grids and the weight gradients' slice counts are the padded shape's.
T4  at an aligned width the ``anyh`` entries are their siblings: step, prepare and act, bit for bit.
T5  the rollout's log-prob and value are the update's: old_kl, kl and clipfrac exactly 0.
T6  ``mlp_layered_minibatch`` equals the native step followed by ``clip_adam_`` in every bit.
tests/test_layered_hidden_host.py shows on the CPU that a correct fp32 computation meets the bars at every case's shape."""
import pytest
import torch

from tests import layered_act_cases as LA
from tests import layered_hidden_cases as LH
from tests import ref64 as R
from tests import test_layered_ragged_fp64_gpu as LRG

pytestmark = pytest.mark.gpu

_Guarded = LRG._Guarded


def _policy(hidden, layers, D, A, cont, sd=None, seed=0):
    """The project's actor_critic on the GPU (the case's weights, or seeded ones moved off their initialisation), its flat bucket and
    its layered layout, taken through ``any_hidden=True``."""
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
    lay = H.mlp_layered_layout(pol, bucket, any_state=True, any_hidden=True)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (D, A, hidden, layers)
    assert bool(lay.get("ragged_hidden")) == (hidden % 32 != 0)
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
@pytest.mark.parametrize("c", LH.STEP_CASES, ids=LH.STEP_IDS)
def test_layered_step_matches_fp64_at_a_ragged_hidden_width(c):
    """Scalars and every gradient tensor of one step, element by element on the scale of the terms behind each element; a second
    launch gives the same bits; nothing past ``n_params`` is written, nothing inside is left unwritten, the parameters stand."""
    data = R.build_case(c)
    ref = R.reference_step(c, data)
    data["ref"] = ref
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    H, _pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    assert lay["ragged_hidden"] is True
    obs, act, rec, idx = R.gpu_inputs(c, data)
    n = lay["n_params"]
    p0 = bucket.flat_param.clone()
    (sc, g), (sc2, g2) = _step(H, obs, act, rec, idx, bucket, lay, c), _step(H, obs, act, rec, idx, bucket, lay, c)
    assert bool(torch.isnan(g[n:]).all()), "the step wrote past n_params"
    assert not bool(torch.isnan(g[:n]).any()), "an entry of the gradient was not written"
    assert torch.equal(bucket.flat_param, p0), "the step wrote into the parameters"
    assert torch.equal(g[:n], g2[:n]) and _same(sc, sc2), "two launches differ"
    R.check_step(c, sc, g[:n], ref, Y, Ys, "layered, ragged hidden: aurppo_mlp_layered_anyh_step_f32")


# ---------------------------------------------------------------------------------- T2: the rollout step
@pytest.mark.parametrize("c", LH.ACT_CASES, ids=LH.ACT_IDS)
def test_layered_act_matches_fp64_at_a_ragged_hidden_width(c):
    data = LA.build(c)
    ref = data["ref"]
    Y, y = LA.yardstick(c, data, "cuda")
    H, pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    assert lay["ragged_hidden"] is True
    N = c.M
    obs, noise = data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous()
    p0 = bucket.flat_param.clone()

    def run(wop=None, **kw):
        ga, gl, gv = _Guarded(*((N, c.A) if c.cont else (N,))), _Guarded(N), _Guarded(N)
        a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, ga.view, gl.view, gv.view, wop=wop, **kw)
        torch.cuda.synchronize()
        assert a is ga.view and lp is gl.view and v is gv.view
        assert ga.guards_intact() and gl.guards_intact() and gv.guards_intact(), "a guard was written"       # (a)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(v).all())
        return a.clone(), lp.clone(), v.clone()

    a, lp, v = run()
    if not c.cont:
        assert torch.equal(a.long().cpu(), ref["action"]), int((a.long().cpu() != ref["action"]).sum())
    m = LA.metrics(c, ref, v, a, lp)
    print(f"\n[layered act, ragged hidden: aurppo_mlp_layered_anyh_act_f32] {R.case_id(c)}: "
          + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items()) + f" (Y {Y:.3e}; moved {data['moved']})")
    for n, x in m.items():
        assert x <= R.MARGIN * Y, (n, x, Y, x / Y)
    for got, first in zip(run(), (a, lp, v)):                                                                # (b)
        assert torch.equal(got, first), "two calls differ"
    wop = H.mlp_layered_prepare(bucket.flat_param, lay)
    for got, first in zip(run(wop), (a, lp, v)):                                                             # (c)
        assert torch.equal(got, first), "prepared weights change the result"
    for got, first in zip(run(wop, paired=True), (a, lp, v)):                                                # (e)
        assert torch.equal(got, first), "the paired step differs from the unpaired one"
    for got, first in zip(run(paired=True), (a, lp, v)):
        assert torch.equal(got, first), "the paired step, preparing its own copies, differs"
    for kw in ({}, dict(paired=True)):                                                                       # (d)
        gv = _Guarded(N)
        a0, lp0, v0 = H.mlp_layered_act(obs, None, bucket.flat_param, lay, value=gv.view, **kw)
        torch.cuda.synchronize()
        assert a0 is None and lp0 is None and torch.equal(v0, v) and gv.guards_intact()
    assert torch.equal(bucket.flat_param, p0)


# ---------------------------------------------------------------------------------- T3: the padded net's bits
def _padded_sd(sd, hidden, Hp):
    """The state dict of the Hp-wide policy whose parameters are ``sd``'s, zeros elsewhere (no other dimension of the shapes used
    here equals the hidden width)."""
    out = {}
    for k, v in sd.items():
        shape = tuple(Hp if s == hidden and not (k == "actor_logstd") else s for s in v.shape)
        t = torch.zeros(shape, dtype=v.dtype)
        t[tuple(slice(0, s) for s in v.shape)] = v
        out[k] = t
    return out


def _real_mask(pol_pad, pol, bucket_pad):
    """True at the padded bucket's positions that hold a parameter of the ragged policy, in the ragged bucket's order."""
    mask = torch.zeros(bucket_pad.flat_param.numel(), dtype=torch.bool, device="cuda")
    pos = 0
    for pp, pr in zip(pol_pad.parameters(), pol.parameters()):
        m = torch.zeros(pp.shape, dtype=torch.bool, device="cuda")
        m[tuple(slice(0, s) for s in pr.shape)] = True
        mask[pos:pos + pp.numel()] = m.reshape(-1)
        pos += pp.numel()
    return mask, pos


@pytest.mark.parametrize("c", [R._mk("layered", 200, 2, 17, 6, True, 257, True, 1),
                               R._mk("layered", 130, 3, 4, 2, False, 65, True, 1),
                               R._mk("layered", 33, 1, 129, 1, True, 1, False, 1),
                               R._mk("layered", 1000, 1, 3, 1, True, 2, True, 1)],
                         ids=["2x200-D17-gauss-M257", "3x130-D4-cat-M65", "1x33-D129-gauss-M1", "1x1000-D3-gauss-M2"])
def test_the_ragged_policy_gives_the_bits_of_its_zero_padded_neighbour_through_the_existing_entries(c):
    data = R.build_case(c)
    Hp = (c.hidden + 31) // 32 * 32
    assert c.hidden not in (c.D, c.A, 1)
    H, pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    Hq, pol_p, bucket_p, lay_p = _policy(Hp, c.layers, c.D, c.A, c.cont, _padded_sd(data["sd"], c.hidden, Hp))
    assert lay["ragged_hidden"] is True and "ragged_hidden" not in lay_p and lay_p["hidden"] == Hp
    mask, n_pad = _real_mask(pol_p, pol, bucket_p)
    n = lay["n_params"]
    assert n_pad == lay_p["n_params"] and int(mask.sum()) == n
    assert torch.equal(bucket_p.flat_param[:n_pad][mask[:n_pad]], bucket.flat_param[:n]), "the two buckets hold the same policy"
    assert bool((bucket_p.flat_param[:n_pad][~mask[:n_pad]] == 0).all())
    obs, act, rec, idx = R.gpu_inputs(c, data)
    sc, g = _step(H, obs, act, rec, idx, bucket, lay, c)
    sc_p, g_p = _step(H, obs, act, rec, idx, bucket_p, lay_p, c)
    assert _same(sc, sc_p), "the nine scalars differ from the padded policy's"
    assert not bool(torch.isnan(g[:n]).any()) and bool(torch.isnan(g[n:]).all())
    assert torch.equal(g_p[:n_pad][mask[:n_pad]], g[:n]), "a gradient entry differs from the padded policy's"
    assert bool((g_p[:n_pad][~mask[:n_pad]] == 0).all()), "the padded policy has a gradient at a pad position"
    # the rollout step over all B rows of the case, unpaired and paired
    gen = torch.Generator(device="cuda").manual_seed(c.seed)
    B = obs.shape[0]
    noise = torch.randn(B, c.A, device="cuda", generator=gen) if c.cont else torch.rand(B, device="cuda", generator=gen)
    for kw in ({}, dict(paired=True)):
        out = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, **kw)
        out_p = H.mlp_layered_act(obs, noise, bucket_p.flat_param, lay_p, **kw)
        torch.cuda.synchronize()
        for name, x, y in zip(("actions", "log-prob", "value"), out, out_p):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y), f"{name} differs from the padded policy's ({kw})"
        v = H.mlp_layered_act(obs, None, bucket.flat_param, lay, **kw)[2]
        assert torch.equal(v, out_p[2])


# ---------------------------------------------------------------------------------- T4: an aligned width
def test_at_an_aligned_width_the_anyh_entries_are_their_siblings(monkeypatch):
    c = R._mk("layered", 256, 2, 17, 6, True, 257, True, 1)
    data = R.build_case(c)
    H, pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    assert "ragged_hidden" not in lay
    forced = dict(lay, ragged_hidden=True)              # the wrappers then call the library's anyh entries with hidden = 256
    called = []
    check = H._check
    monkeypatch.setattr(H, "_check", lambda rc, name: (called.append(name), check(rc, name))[1])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    sc, g = _step(H, obs, act, rec, idx, bucket, lay, c)
    sc_a, g_a = _step(H, obs, act, rec, idx, bucket, forced, c)
    n = lay["n_params"]
    assert _same(sc, sc_a) and torch.equal(g[:n], g_a[:n]) and bool(torch.isnan(g_a[n:]).all())
    H._layered_wop_cache.clear()
    buf = H.mlp_layered_prepare(bucket.flat_param, lay)
    buf.zero_()                                         # (a copy's group of slack is never written)
    wop = H.mlp_layered_prepare(bucket.flat_param, lay).clone()
    buf.zero_()
    wop_a = H.mlp_layered_prepare(bucket.flat_param, forced)        # the same shape: the same buffer
    torch.cuda.synchronize()
    assert wop_a is buf and torch.equal(wop, wop_a) and int((wop != 0).sum()) > 0
    noise = torch.randn(obs.shape[0], c.A, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for kw in ({}, dict(paired=True)):
        out = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, **kw)
        out_a = H.mlp_layered_act(obs, noise, bucket.flat_param, forced, wop=wop_a, **kw)
        torch.cuda.synchronize()
        for x, y in zip(out, out_a):
            assert torch.equal(x, y)
    H._layered_wop_cache.clear()
    assert [e for e in called if "anyh" in e] == ["aurppo_mlp_layered_anyh_step_f32", "aurppo_mlp_layered_anyh_prep_f32",
                                                  "aurppo_mlp_layered_anyh_act_f32", "aurppo_mlp_layered_anyh_act_paired_f32"]


# ---------------------------------------------------------------------------------- T5: the rollout's log-prob is the update's
@pytest.mark.parametrize("hidden,layers,D,A,cont,N,M,packed", [(200, 2, 17, 6, True, 513, 300, False), (130, 3, 11, 3, True, 257, 100, True)],
                         ids=["2x200-D17", "3x130-D11-packed"])
def test_the_rollouts_logp_and_value_are_the_updates_at_a_ragged_hidden_width(hidden, layers, D, A, cont, N, M, packed):
    """``mlp_layered_act`` over N rows, then ``mlp_layered_step_native`` over a permutation slice of them with old_logp / old_v from the
    rollout: the ratio is exp(0) for every sample, so old_kl, kl and clipfrac are exactly 0."""
    H, pol, bucket, lay = _policy(hidden, layers, D, A, cont, seed=hidden + N)
    g = torch.Generator(device="cuda").manual_seed(N * 7 + M)
    obs = torch.randn(N, D, device="cuda", generator=g)
    noise = torch.randn(N, A, device="cuda", generator=g) if cont else torch.rand(N, device="cuda", generator=g)
    a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay)
    rec = torch.stack([lp, torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g), v], 1).contiguous()
    idx = torch.randperm(N, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    acts = a
    if packed:
        rec, acts = H.pack_records(rec, a.reshape(N, -1)), None
    grad = torch.empty_like(bucket.flat_grad)
    sc = H.mlp_layered_step_native(obs, acts, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED).cpu()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(grad[:lay["n_params"]]).all())
    print(f"\n{layers} x {hidden}, D {D}: old_kl {float(sc[H.S_OLD_KL])!r}, kl {float(sc[H.S_KL])!r}, clipfrac {float(sc[H.S_CLIPFRAC])!r}")
    assert float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0
    # the value took part too: the clipped value loss sees v - old_v == 0, so vl = 0.5 * mean((v - ret)^2) exactly as un-clipped
    sc_u = H.mlp_layered_step_native(obs, acts, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_RETURNS).cpu()
    assert float(sc_u[H.S_VL]) == float(sc[H.S_VL])


# ---------------------------------------------------------------------------------- T6: the minibatch call
def _warm(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return 0.01 * torch.randn(n, device="cuda", generator=g), 1e-4 * torch.rand(n, device="cuda", generator=g)


def test_minibatch_equals_step_then_clip_adam_at_a_ragged_hidden_width():
    c = R._mk("layered", 200, 2, 17, 6, True, 257, True, 1)
    data = R.build_case(c)
    H, _pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    N = lay["n_params"]                             # buffers of exactly n_params floats: clip_adam_ then covers [0, n_params) too
    p0 = bucket.flat_param[:N].clone()
    knobs = (R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    lr = torch.tensor([2.5e-4], device="cuda")
    outs = []
    for fused in (False, True):
        p, grad = p0.clone(), torch.full((N,), float("nan"), device="cuda")
        m, v = _warm(N, c.seed)
        t, norm, sc = torch.tensor([1000.0], device="cuda"), torch.full((1,), float("nan"), device="cuda"), torch.empty(9, device="cuda")
        if fused:
            H.mlp_layered_minibatch(obs, act, rec, idx, p, lay, grad, *knobs, sc, m, v, lr, t, 0.5, (0.9, 0.999), 1e-5, norm)
        else:
            H.mlp_layered_step_native(obs, act, rec, idx, p, lay, grad, *knobs, sc)
            H.clip_adam_(p, grad, m, v, lr, t, 0.5, betas=(0.9, 0.999), eps=1e-5, out_norm=norm)
        torch.cuda.synchronize()
        outs.append(dict(p=p, grad=grad, m=m, v=v, t=t, norm=norm, sc=torch.nan_to_num(sc, nan=-7.0)))
    a, b = outs
    assert float(a["t"]) == 1001.0 and bool(torch.isfinite(a["p"]).all()) and not torch.equal(a["p"], p0)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between the minibatch call and step + clip_adam_"
