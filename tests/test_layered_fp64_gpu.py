"""GPU: the layered PPO step (hip_ops.mlp_layered_step: k_linear / k_linear_wgrad a layer at a time with the gather in the first
product, K13 -- csrc/head.hip -- behind the last) for the MLP policies wider than the fused kernels, against the fp64 reference of
tests/ref64.py used as it is: the same inputs (no sample within BRANCH_EPS of a decision, nothing excluded), metric, yardstick (plain
PyTorch fp32 autograd on the GPU) and bars (MARGIN, MARGIN_TINY_M, MARGIN_SCALARS) as the fused steps in test_mlp_fp64_gpu.py.
tests/test_layered_host.py shows on the CPU that a correct fp32 computation meets these bars at every case's shape."""
import pytest
import torch

from tests import layered_cases as LC
from tests import ref64 as R

pytestmark = pytest.mark.gpu


def _policy(c, sd):
    """The project's actor_critic with the case's weights on the GPU, its flat bucket and its layered layout."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    pol.load_state_dict(sd)
    pol = pol.cuda()
    bucket = FlatBucket(pol.parameters())
    assert H.mlp_layout(pol, bucket) is None
    lay = H.mlp_layered_layout(pol, bucket)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (c.D, c.A, c.hidden, c.layers)
    assert [n for n, _ in pol.named_parameters()] == R.param_names(R.make_net(sd)), "FlatBucket order"
    return pol, bucket, lay


@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_layered_step_matches_fp64(c):
    """Scalars and every gradient tensor of one step, element by element on the scale of the terms behind each element; a second
    launch gives the same bits; nothing past ``n_params`` is written."""
    from aur_ppo_amd import hip_ops as H
    data = R.build_case(c)
    ref = R.reference_step(c, data)
    data["ref"] = ref
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    _pol, bucket, lay = _policy(c, data["sd"])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    n = lay["n_params"]
    runs = []
    for _ in range(2):
        g = torch.full((bucket.flat_grad.numel() + 64,), float("nan"), device="cuda")
        sc = H.mlp_layered_step(obs, act, rec, idx, bucket.flat_param, lay, g, R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"],
                                c.norm_adv, c.vmode)
        torch.cuda.synchronize()
        runs.append((sc.clone(), g))
    (sc, g), (sc2, g2) = runs
    assert bool(torch.isnan(g[n:]).all()), "the step wrote past n_params"
    assert torch.equal(g[:n], g2[:n]) and torch.equal(torch.nan_to_num(sc, nan=-7.0), torch.nan_to_num(sc2, nan=-7.0)), "two launches differ"
    R.check_step(c, sc, g[:n], ref, Y, Ys, "layered: k_linear + K13 k_head_ppo")


@pytest.mark.parametrize("cont", [True, False], ids=["gauss", "cat"])
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("Hd", [32, 1024])
def test_head_kernel_in_place_equals_separate_output(Hd, M, cont):
    """K13 alone on random activations: gz written over its h == gz written to a buffer of its own, bit for bit, and so is
    everything else it leaves (scalars, head / logstd / last-layer bias gradients)."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    A, D = 6, 16
    torch.manual_seed(Hd + M)
    pol = actor_critic(D, (A,) if cont else A, Hd, 1, 0.0, cont).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    bucket = FlatBucket(pol.parameters())
    seq, n, _D, _A, _cont, NL, _Hd = H._mlp_structure(pol, bucket)
    lay = dict(offsets=seq, n_params=n, D=D, A=A, continuous=cont, hidden=Hd, num_layers=NL, layered=True)
    g = torch.Generator(device="cuda").manual_seed(Hd * 3 + M)
    B = M + 37
    hA = torch.tanh(torch.randn(M, Hd, device="cuda", generator=g))
    hC = torch.tanh(torch.randn(M, Hd, device="cuda", generator=g))
    act = torch.randn(B, A, device="cuda", generator=g) if cont else torch.randint(0, A, (B,), device="cuda", generator=g).float()
    rec = torch.stack([-3 + 0.2 * torch.randn(B, device="cuda", generator=g), 2 * torch.randn(B, device="cuda", generator=g),
                       torch.randn(B, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)], 1).contiguous()
    idx = torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    # old log-prob and old value of the minibatch's samples close to the new ones: the ratio and the value stay inside the clip, so every
    # sample sends a gradient to both nets
    with torch.no_grad():
        li = idx.long()
        out = pol.actor.net[2](hA)
        if cont:
            ls = pol.actor_logstd.expand_as(out)
            lp = (-((act[li] - out) ** 2) / (2 * torch.exp(ls) ** 2) - ls - 0.9189385332046727).sum(1)
        else:
            lp = torch.log_softmax(out, 1).gather(1, act[li].long()[:, None])[:, 0]
        v = pol.critic.net[2](hC).view(-1)
        rec[li, 0] = lp + 0.05 * torch.randn(M, device="cuda", generator=g)
        rec[li, 2] = v + torch.randn(M, device="cuda", generator=g)
        rec[li, 3] = v + 0.05 * torch.randn(M, device="cuda", generator=g)
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
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    ga, gc, grad, sc = outs[0]
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gc).all()) and float(ga.abs().max()) > 0 and float(gc.abs().max()) > 0
    # written: the heads, actor_logstd and the two last-layer biases; the first layer's weights are not K13's
    hl = H.head_layout(lay)
    assert bool((grad[hl[0]:hl[0] + A * Hd] != -7.0).all()) and bool((grad[hl[5]:hl[5] + Hd] != -7.0).all())
    assert bool((grad[seq[0]:seq[0] + Hd * D] == -7.0).all())
    # the last hidden layer's bias gradient is the column sum of gz
    torch.testing.assert_close(grad[hl[5]:hl[5] + Hd], ga.sum(0), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(grad[hl[6]:hl[6] + Hd], gc.sum(0), rtol=1e-4, atol=1e-6)
