"""GPU: every build of the fused MLP step (K7 k_mlp_step3 / k_mlp_step2, K7w ids 1 / 3 / 2) and the rollout step (K8 / K8w) against
the fp64 reference of tests/ref64.py, at the level of fp32 rounding.

The bar of every check is a margin x Y, where Y is what plain PyTorch fp32 autograd on the GPU loses against fp64 on the same case and
the same metric (error over the sum of the absolute terms behind each number).  The margin is ``ref64.MARGIN`` = 2 for every gradient
tensor at M >= 31, every per-sample forward value and the rollout step; minibatches of fewer than 31 samples and the nine scalars,
whose Y is the rounding of a handful of numbers, have class margins of their own (``MARGIN_TINY_M``, ``MARGIN_SCALARS``).  DESIGN's
parity section derives all three from profiles/mlp_fp64_table.txt (``tools/mlp_fp64_table.py`` prints it) and from a second correct fp32
formulation on the CPU, and lists the wrong kernels the bars reject (tests/test_ref64_host.py shows both on the CPU).  The inputs keep every sample at least ``ref64.BRANCH_EPS`` away from every branch
of the loss, so that nothing is excluded anywhere: no skip, no agreement fraction.  Each test prints the kernel it ran (``-s``)."""
import numpy as np
import pytest
import torch

from tests import ref64 as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(c):
    """Inputs, fp64 reference and the fp32 torch yardstick of a case, computed once."""
    if c not in _CACHE:
        data = R.build_case(c)
        data["ref"] = R.reference_step(c, data)
        data["Y"], data["Ys"], _ = R.yardstick_step(c, data, "cuda")
        data["gpu"] = R.gpu_inputs(c, data)
        del data["net64"]
        _CACHE[c] = data
    return _CACHE[c]


def _check_step(label, c, sc, g, ref, Y, Ys):
    R.check_step(c, sc, g, ref, Y, Ys, label)


_STEP = [(c, k) for c in R.K7_CASES + R.K7W_CASES for k in R.kernels_for(c)]


@pytest.mark.parametrize("static", [0, 1], ids=["counter", "static-tiles"])
@pytest.mark.parametrize("c,k", _STEP, ids=[f"{k.name}-{R.case_id(c)}" for c, k in _STEP])
def test_step_matches_fp64(c, k, static, monkeypatch):
    """Scalars and every gradient tensor of one launch, element by element on the scale of the terms behind each element."""
    data = _case(c)
    label = R.select_kernel(c, k, static, monkeypatch.setenv)
    pbl = R.gpu_policy(c, data["sd"])
    sc, g = R.kernel_step(c, data, pbl)
    torch.cuda.synchronize()
    _check_step(label, c, sc, g, data["ref"], data["Y"], data["Ys"])


_FWD = [(c, k) for c in R.FWD_CASES for k in R.kernels_for(c)]


@pytest.mark.parametrize("static", [0, 1], ids=["counter", "static-tiles"])
@pytest.mark.parametrize("c,k", _FWD, ids=[f"{k.name}-{R.case_id(c)}" for c, k in _FWD])
def test_forward_per_sample_matches_fp64(c, k, static, monkeypatch):
    """K7 / K7w have no per-sample outputs; minibatches of ONE sample expose them: with old_logp = 0 ``old_approx_kl`` is -logp,
    ``entropy`` is the sample's entropy, and with the un-clipped value loss against a return of 0 and vf_coef = 1 the critic head's
    bias gradient is the value.  64 samples per kernel, each on the scale of the head's product behind it."""
    from aur_ppo_amd import hip_ops as H
    data = R.build_case(c)
    li = data["idx"].long()
    obs, act = data["obs"][li], data["act"][li]
    rec = torch.zeros(c.M, 4)
    rec[:, 1] = 1.0
    ref = R.run_step(data["net64"], obs.double(), act.double(), rec.double(), 0.2, 0.01, 1.0, False, 0, scales=True)
    net32 = R.make_net(data["sd"], torch.float32, "cuda")
    with torch.no_grad():
        _, lp_t, ent_t, v_t = net32.evaluate(obs.cuda(), act.cuda() if c.cont else act.cuda().long())
    y = R.forward_metrics(lp_t, ent_t, v_t, ref)
    Y = max(y.values())
    label = R.select_kernel(c, k, static, monkeypatch.setenv)
    _pol, bucket, lay = R.gpu_policy(c, data["sd"])
    b3c = lay["offsets"][-2]                          # critic head bias (last entry before actor_logstd in both layouts)
    obs_g, act_g, rec_g = obs.cuda().contiguous(), act.cuda().contiguous(), rec.cuda().contiguous()
    g = torch.empty_like(bucket.flat_grad)
    lp, ent, val = [], [], []
    for i in range(c.M):
        idx = torch.tensor([i], device="cuda", dtype=torch.int32)
        sc = H.mlp_ppo_step(obs_g, act_g, rec_g, idx, bucket.flat_param, lay, g, 0.2, 0.01, 1.0, False, H.VLOSS_RETURNS).cpu()
        lp.append(-float(sc[H.S_OLD_KL]))
        ent.append(float(sc[H.S_ENT]))
        val.append(float(g[b3c]))
    m = R.forward_metrics(torch.tensor(lp), torch.tensor(ent), torch.tensor(val), ref)
    print(f"\n[{label}] {R.case_id(c)}: " + ", ".join(f"{n} {v:.3e} = {v / Y:.2f} x Y" for n, v in m.items()) + f" (Y {Y:.3e}; torch fp32 {y})")
    for n, v in m.items():
        assert v <= R.MARGIN * Y, (label, n, v, Y, v / Y)


# ---------------------------------------------------------------------------------- the chained paths
_CHAIN = [(R._mk("k7", 64, 2, 64, 6, True, 300, True, 1), "minibatch"), (R._mk("k7", 64, 2, 6, 5, False, 300, True, 1), "minibatch"),
          (R._mk("k7", 64, 2, 17, 6, True, 300, True, 1), "grad+apply"), (R._mk("k7w", 128, 3, 64, 6, True, 300, True, 1), "handed-over"),
          (R._mk("k7w", 64, 3, 24, 6, True, 300, True, 1), "handed-over"), (R._mk("k7w", 96, 2, 100, 4, False, 300, True, 1), "prepare-each-call")]
_CHAIN = [(c, mode, k) for c, mode in _CHAIN for k in R.kernels_for(c)]


@pytest.mark.parametrize("c,mode,k", _CHAIN, ids=[f"{k.name}-{mode}-{R.case_id(c)}" for c, mode, k in _CHAIN])
def test_chained_minibatches_match_fp64_at_the_parameters_each_call_saw(c, mode, k, monkeypatch):
    """``mlp_ppo_minibatch`` (and ``mlp_ppo_grad`` + ``mlp_ppo_apply``, and the wide twin with and without hand-over) over three
    consecutive minibatches, the last one ragged: the gradient each call leaves in ``g_out`` against the fp64 gradient at the
    parameters that call read -- so the operand copies the optimizer launch prepares for the next call are held to the same bar.
    Before each call the parameters are read back and that slice's records are made margin-safe for them (old_logp / ret / old_v
    only: the advantage statistics a previous call may have prepared do not change)."""
    from aur_ppo_amd import hip_ops as H
    rs = np.random.RandomState(c.seed)
    sd = R.make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs)
    B, M = 2 * c.M + 137, c.M
    obs = R.make_obs(B, c.D, "normal", rs)
    act = torch.from_numpy(rs.standard_normal((B, c.A)).astype(np.float32) if c.cont else rs.randint(0, c.A, size=B).astype(np.float32))
    net64 = R.make_net(sd)
    with torch.no_grad():
        _, lp0, _, v0 = net64.evaluate(obs.double(), act.double() if c.cont else act.long())
    rec = torch.stack([lp0 + 0.2 * torch.from_numpy(rs.standard_normal(B)), 2 * torch.from_numpy(rs.standard_normal(B)),
                       v0.reshape(-1) + torch.from_numpy(rs.standard_normal(B)), v0.reshape(-1) + 0.25 * torch.from_numpy(rs.standard_normal(B))], 1).float()
    perm = torch.from_numpy(rs.permutation(B).astype(np.int32))
    slices = [perm[s:s + M] for s in range(0, B, M)]
    assert [s.numel() for s in slices] == [M, M, 137]
    label = R.select_kernel(c, k, 0, monkeypatch.setenv)
    _pol, bucket, lay = R.gpu_policy(c, sd)
    n, nb = lay["n_params"], bucket.flat_param.numel()
    obs_g, act_g, rec_g = obs.cuda().contiguous(), act.cuda().contiguous(), rec.cuda().contiguous()
    sl_g = [s.cuda() for s in slices]
    m_, v_, g = (torch.zeros(nb, device="cuda") for _ in range(3))
    lr, t = torch.full((1,), 3e-3, device="cuda"), torch.zeros(1, device="cuda")
    sc, norms = torch.zeros(3, 9, device="cuda"), torch.zeros(3, device="cuda")
    names = R.param_names(net64)
    p_first = bucket.flat_param[:n].clone()
    for i, idx in enumerate(slices):
        # the parameters this call will read, back on the host
        flat = bucket.flat_param[:n].detach().cpu()
        sd_i, off = {}, 0
        for nm, p in zip(names, net64.parameters()):
            sd_i[nm] = flat[off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
        net_i = R.make_net(sd_i)
        li = idx.long()
        with torch.no_grad():
            _, lp, _, v = net_i.evaluate(obs[li].double(), act[li].double() if c.cont else act[li].long())
        R.make_records_safe(lp, v.reshape(-1), rec, idx, R.HYPER["clip"], True, 1)
        rec_g[sl_g[i].long()] = rec[li].cuda()
        data = dict(sd=sd_i, net64=net_i, obs=obs, act=act, rec=rec, idx=idx)
        data["ref"] = R.reference_step(c, data)
        Y, Ys, _ = R.yardstick_step(c, data, "cuda")
        nxt = sl_g[i + 1] if i + 1 < len(slices) else None
        args = (obs_g, act_g, rec_g, sl_g[i], bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1, sc[i])
        if mode == "grad+apply":
            H.mlp_ppo_grad(*args, t, chained=i > 0)
            torch.cuda.synchronize()
            got = g[:n].clone()
            H.mlp_ppo_apply(bucket.flat_param, g, m_, v_, lay, lr, t, 1e9, (0.9, 0.999), 1e-5, norms[i:i + 1], rec=rec_g, next_idx=nxt)
        else:
            hand = mode != "prepare-each-call"
            H.mlp_ppo_minibatch(*args, m_, v_, lr, t, 1e9, (0.9, 0.999), 1e-5, norms[i:i + 1], next_idx=nxt if hand else None,
                                chained=hand and i > 0)
            torch.cuda.synchronize()
            got = g[:n].clone()           # max_norm = 1e9: the clip leaves the gradient as the step wrote it
        _check_step(f"{label} {mode} call {i}", c, sc[i], got, data["ref"], Y, Ys)
    assert float(t) == 3 and float((bucket.flat_param[:n] - p_first).abs().max()) > 1e-3      # the run did move the parameters


# ---------------------------------------------------------------------------------- K8 / K8w: the rollout step
_ACT = [(R._mk("k7", 64, 2, 64, 6, True, 4096, False, 0), "normal"), (R._mk("k7", 64, 2, 4, 2, False, 77, False, 0), "normal"),
        (R._mk("k7", 64, 2, 17, 16, False, 4096, False, 0), "scaled"), (R._mk("k7", 64, 2, 3, 1, True, 1, False, 0), "bf16half"),
        (R._mk("k7", 64, 2, 15, 12, True, 33, False, 0), "scaled"), (R._mk("k7w", 128, 3, 128, 2, False, 4096, False, 0), "normal"),
        (R._mk("k7w", 32, 1, 5, 5, False, 33, False, 0), "bf16half"), (R._mk("k7w", 100, 2, 65, 16, True, 1000, False, 0), "scaled"),
        (R._mk("k7w", 64, 3, 16, 16, False, 256, False, 0), "normal"), (R._mk("k7w", 7, 1, 1, 1, True, 1, False, 0), "normal"),
        (R._mk("k7w", 96, 2, 127, 6, True, 65, False, 0), "bf16half")]


@pytest.mark.parametrize("c,regime", _ACT, ids=[("K8-" if c.kind == "k7" else "K8w-") + R.case_id(c._replace(regime=r)) for c, r in _ACT])
def test_act_kernel_matches_fp64(c, regime):
    """Value, action and log-prob per sample.  Categorical head: the uniform draws keep BRANCH_EPS away from every edge of the fp64 CDF,
    so the sampled index must be EQUAL for every sample."""
    from aur_ppo_amd import hip_ops as H
    rs = np.random.RandomState(c.seed + 1)
    sd = R.make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs, 1e-3 if regime == "scaled" else 1.0)
    N = c.M
    obs = R.make_obs(N, c.D, regime, rs)
    net64 = R.make_net(sd)
    if c.cont:
        noise = torch.from_numpy(rs.standard_normal((N, c.A)).astype(np.float32))
    else:
        noise = torch.from_numpy(rs.random_sample(N).astype(np.float32))
        R.safe_uniform(net64, obs, noise)
    ref = R.act_reference(net64, obs, noise)
    # yardstick: the same formulas in plain fp32 torch on the GPU
    net32 = R.make_net(sd, torch.float32, "cuda")
    with torch.no_grad():
        o, z = obs.cuda(), noise.cuda()
        v_t = net32.value(o)
        if c.cont:
            a_t = net32.actor(o) + net32.actor_logstd.exp() * z
            _, lp_t, _, _ = net32.evaluate(o, a_t)
        else:
            _, lp_t, _, _ = net32.evaluate(o, ref["action"].cuda())

    def metrics(v, a, lp):
        out = {"value": float(((v.double().cpu() - ref["value"]).abs() / ref["fwd_scales"]["value"]).max()),
               "logp": float(((lp.double().cpu() - ref["logp"]).abs() / ref["fwd_scales"]["logp"]).max())}
        if c.cont:
            out["action"] = float(((a.double().cpu() - ref["action"]).abs() / ref["fwd_scales"]["action"]).max())
        return out
    y = metrics(v_t, a_t if c.cont else None, lp_t)
    Y = max(max(y.values()), R.ULP32)
    _pol, bucket, lay = R.gpu_policy(c, sd)
    a, lp, v = H.mlp_act(obs.cuda().contiguous(), noise.cuda().contiguous(), bucket.flat_param, lay)
    torch.cuda.synchronize()
    if not c.cont:
        assert torch.equal(a.long().cpu(), ref["action"]), int((a.long().cpu() != ref["action"]).sum())
    m = metrics(v, a, lp)
    print(f"\n[{'K8w' if lay['wide'] else 'K8'}] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items()) + f" (Y {Y:.3e})")
    for n, x in m.items():
        assert x <= R.MARGIN * Y, (n, x, Y, x / Y)
    _, _, v2 = H.mlp_act(obs.cuda().contiguous(), None, bucket.flat_param, lay)      # value-only mode (the bootstrap)
    assert torch.equal(v2, v)
