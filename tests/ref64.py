"""fp64 reference of one fused MLP minibatch step (K7 / K7w) and of the rollout step (K8 / K8w), the inputs the fp64 tests
feed the kernels, and the metric they are judged on.  A plain helper module (no tests in it); DESIGN's parity section
derives the bars.

What is here
  * ``make_net``: the oracle's actor-critic (``oracle.ppo_oracle.make_actor_critic``) loaded with a state dict, in any dtype.
  * ``run_step``: evaluate + the loss of src/ppo.py:225-264 in torch ops + autograd, in the dtype of its inputs.  In float64
    on the CPU it is the reference; in float32 (on the GPU, or on the CPU for the host tests) it is the YARDSTICK: what a
    plain fp32 computation of the same step loses against fp64.  The hyper-parameters are the fp32 roundings the kernels
    and the oracle use (``float32(1 - clip)``, ``float32(1 + clip)``, ``float32(clip)``, the two coefficients).
  * ``grad_metrics`` / ``scalar_metrics`` / ``forward_metrics``: error against fp64 on the scale of the terms behind each
    number (for dW = d^T x the scale is |d|^T |x|), so that a gradient that cancels needs no floor.
  * ``build_case``: weights, observations, actions, records and index of a case, all from numpy's legacy generator on the
    CPU, with the records moved until NO sample of the minibatch is within ``BRANCH_EPS`` of a decision of the loss.
  * ``act_reference`` / ``safe_uniform``: the same for the rollout step.
  * ``make_emulated_net``: the step's matrix products formed from three bf16 planes (csrc/bf16x3.h's opening comment) with a
    chosen set of the nine plane products per role, for the host tests that show which wrong kernels the bars reject.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch
from torch import nn

from oracle import ppo_oracle as O

# Bars: metric <= margin * Y, Y = plain fp32 torch on the same case and metric.  DESIGN's parity section derives the three figures
# (profiles/mlp_fp64_table.txt for the kernels; tests/test_ref64_host.py re-measures the two class margins on the CPU).
MARGIN = 2.0               # gradient tensors at M >= TINY_M, per-sample forward values, the rollout step
TINY_M = 31                # below this a minibatch's Y is the rounding of a handful of samples: a draw, not a level
MARGIN_TINY_M = 64.0       # gradient tensors at M < TINY_M
MARGIN_SCALARS = 16.0      # the nine scalars (Y: the worst of the nine in fp32 torch, at least one fp32 ulp of the scale)
BRANCH_EPS = 1e-4          # no sample may sit closer than this to a branch point (a condition on the inputs)
ULP32 = 2.0 ** -24
SCALAR_NAMES = ["loss", "pg", "vl", "ent", "old_kl", "kl", "clipfrac", "adv_mean", "adv_std"]
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the policy
def net_shape(sd):
    """(D, A, hidden, layers, continuous) of an actor_critic state dict."""
    layers = sum(1 for k in sd if k.startswith("actor.net.") and k.endswith(".weight")) - 1
    hidden, D = sd["actor.net.0.weight"].shape
    A = sd[f"actor.net.{2 * layers}.weight"].shape[0]
    return int(D), int(A), int(hidden), int(layers), "actor_logstd" in sd


def make_net(sd, dtype=torch.float64, device="cpu"):
    D, A, hidden, layers, cont = net_shape(sd)
    net = O.make_actor_critic(D, (A,) if cont else A, hidden, layers, cont)
    net.load_state_dict({k: v.detach().cpu().float() for k, v in sd.items()})
    return net.to(dtype=dtype, device=device)


def param_names(net):
    """Parameter names in FlatBucket order (``parameters()`` order: actor_logstd first, then actor, then critic)."""
    return [n for n, _ in net.named_parameters()]


# ------------------------------------------------------------------------------------------------ the step
def loss_terms(logp, ent, v, rec, clip, ent_coef, vf_coef, norm_adv, vmode):
    """src/ppo.py:225-264 with torch ops in the dtype of its inputs; per-sample terms and the nine scalars."""
    c, lo, hi, ec, vc = f32(clip), f32(1 - clip), f32(1 + clip), f32(ent_coef), f32(vf_coef)
    old_lp, adv, ret, old_v = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    M = logp.shape[0]
    v = v.reshape(-1)
    lr = logp - old_lp                                             # ppo.py:226
    ratio = lr.exp()
    kl_t = (ratio - 1) - lr
    cf_t = ((ratio - 1.0).abs() > c).to(logp.dtype)
    mean = adv.mean()
    std = adv.std() if M > 1 else torch.full_like(mean, float("nan"))      # ddof = 1
    an = (adv - mean) / (std + 1e-8) if norm_adv else adv          # ppo.py:238-239
    l1 = -an * ratio
    l2 = -an * torch.clamp(ratio, lo, hi)
    pg_t = torch.max(l1, l2)                                       # ppo.py:245
    if vmode == O.VLOSS_CLIPPED:                                   # ppo.py:250-259
        vu = (v - ret) ** 2
        vcl = old_v + torch.clamp(v - old_v, -c, c)
        vcc = (vcl - ret) ** 2
        vl_t = torch.max(vu, vcc)
    elif vmode == O.VLOSS_RETURNS:                                 # robot_ppo.py:390
        vl_t = (v - ret) ** 2
    else:                                                          # ppo.py:261
        vl_t = (v - old_v) ** 2
    pg, vl, e = pg_t.mean(), 0.5 * vl_t.mean(), ent.mean()
    loss = pg - ec * e + vl * vc                                   # ppo.py:264
    sc = torch.stack([loss, pg, vl, e, (-lr).mean(), kl_t.mean(), cf_t.mean(), mean, std]).detach()
    # the mean of the absolute terms each scalar averages (clipfrac is a count: its terms are 0 / 1)
    s_pg, s_vl, s_e = pg_t.abs().mean(), 0.5 * vl_t.abs().mean(), ent.abs().mean()
    ssc = torch.stack([s_pg + ec * s_e + vc * s_vl, s_pg, s_vl, s_e, lr.abs().mean(), ((ratio - 1).abs() + lr.abs()).mean(),
                       cf_t.mean(), adv.abs().mean(), (adv * adv).mean().sqrt()]).detach()
    return loss, sc, ssc


def run_step(net, obs, act, rec, clip, ent_coef, vf_coef, norm_adv, vmode, scales=False):
    """One minibatch step on gathered rows ``obs`` (M, D), ``act`` (M, A) / (M,), ``rec`` (M, 4) = {old_logp, adv, ret, old_v},
    all in the dtype and on the device of ``net``.  Returns a dict: ``scalars`` (9, the library's order), ``grads`` (list of
    tensors in FlatBucket order), ``flat``, ``logp`` / ``ent`` / ``value`` per sample, and with ``scales=True`` (the fp64
    run) ``grad_scales`` (same shapes as grads), ``scalar_scales`` (9) and ``fwd_scales`` (logp, ent, value per sample)."""
    for p in net.parameters():
        p.grad = None
    saved, hooks = {}, []
    if scales:
        def hook(name):
            def fn(_m, inp, out):
                out.retain_grad()
                saved[name] = (inp[0].detach(), out)
            return fn
        for name, mod in net.named_modules():
            if isinstance(mod, nn.Linear) or getattr(mod, "is_linear", False):
                hooks.append(mod.register_forward_hook(hook(name)))
    a_in = act if net.continuous else act.reshape(-1).long()
    _, logp, ent, v = net.evaluate(obs, a_in)
    if scales:
        logp.retain_grad()
    loss, sc, ssc = loss_terms(logp, ent, v, rec, clip, ent_coef, vf_coef, norm_adv, vmode)
    loss.backward()
    for h in hooks:
        h.remove()
    names = param_names(net)
    grads = [p.grad.detach() for p in net.parameters()]
    out = dict(scalars=sc, names=names, grads=grads, flat=torch.cat([g.reshape(-1) for g in grads]),
               logp=logp.detach(), ent=ent.detach(), value=v.detach().reshape(-1))
    if not scales:
        return out
    M = obs.shape[0]
    gs = []
    for n in names:
        if n == "actor_logstd":
            # per-sample term of d loss / d logstd_j: g_logp_s * (z_sj^2 - 1) from the log-prob, -ent_coef / M from the entropy
            mu = saved[_head(net, "actor")][1].detach()
            z = (act - mu) / net.actor_logstd.detach().exp()
            gs.append((logp.grad[:, None] * (z * z - 1) - f32(ent_coef) / M).abs().sum(0, keepdim=True))
            continue
        mod, kind = n.rsplit(".", 1)
        x, y = saved[mod]
        d = y.grad.abs()
        gs.append(d.t() @ x.abs() if kind == "weight" else d.sum(0))
    out.update(grad_scales=gs, scalar_scales=ssc, fwd_scales=_forward_scales(net, saved, act))
    return out


def _head(net, which):
    L = len(getattr(net, which).net) - 1
    return f"{which}.net.{L}"


def _forward_scales(net, saved, act):
    """Per sample, the scale of log-prob, entropy and value: the head's product on the scale sum_k |h_k| |w_k| (+ |b|),
    carried through the derivative of the quantity in the head's outputs, plus the absolute terms of its own sum."""
    def head_scale(which):
        mod = dict(net.named_modules())[_head(net, which)]
        h = saved[_head(net, which)][0]
        return h.abs() @ mod.weight.detach().abs().t() + mod.bias.detach().abs()
    s_mu, s_v = head_scale("actor"), head_scale("critic").reshape(-1)
    mu = saved[_head(net, "actor")][1].detach()
    if net.continuous:
        logstd = net.actor_logstd.detach().expand_as(mu)
        std = logstd.exp()
        z = (act - mu) / std
        s_lp = ((z / std).abs() * s_mu).sum(1) + (0.5 * z * z + logstd.abs() + _HALF_LOG_2PI).sum(1)
        s_ent = (0.5 + _HALF_LOG_2PI + logstd).abs().sum(1)
    else:
        a = act.reshape(-1).long()
        lse = mu.logsumexp(1, keepdim=True)
        lp_all = mu - lse
        p = lp_all.exp()
        H = -(p * lp_all).sum(1, keepdim=True)
        onehot = torch.zeros_like(p).scatter_(1, a[:, None], 1.0)
        s_lp = ((onehot - p).abs() * s_mu).sum(1) + mu.gather(1, a[:, None])[:, 0].abs() + lse[:, 0].abs()
        s_ent = ((p * (lp_all + H)).abs() * s_mu).sum(1) + (p * lp_all).abs().sum(1)
    return dict(logp=s_lp, ent=s_ent, value=s_v)


# ------------------------------------------------------------------------------------------------ metrics
def grad_metrics(flat, ref):
    """{parameter name: max over its elements of |g - g64| / S} for a flat gradient in FlatBucket order."""
    flat = torch.as_tensor(flat).detach().double().cpu().reshape(-1)
    out, off = collections.OrderedDict(), 0
    for n, g64, S in zip(ref["names"], ref["grads"], ref["grad_scales"]):
        k = g64.numel()
        g = flat[off:off + k].view_as(g64)
        assert bool(torch.isfinite(g).all()), f"{n}: non-finite gradient"
        out[n] = float(((g - g64).abs() / S.clamp_min(1e-300)).max())
        off += k
    return out


def scalar_metrics(sc, ref):
    """{scalar name: |s - s64| / scale}.  ``adv_std`` of a one-sample minibatch is NaN on both sides (metric 0)."""
    sc = torch.as_tensor(sc).detach().double().cpu().reshape(-1)
    out = collections.OrderedDict()
    for i, n in enumerate(SCALAR_NAMES):
        a, b, s = float(sc[i]), float(ref["scalars"][i]), float(ref["scalar_scales"][i])
        if math.isnan(b):
            assert math.isnan(a), f"{n}: expected NaN, got {a}"
            out[n] = 0.0
        else:
            assert math.isfinite(a), f"{n}: {a}"
            out[n] = abs(a - b) / s if s > 0 else (0.0 if a == b else float("inf"))
    return out


def forward_metrics(logp, ent, value, ref):
    """{logp / ent / value: max over samples of |x - x64| / scale}."""
    out = collections.OrderedDict()
    for n, x in (("logp", logp), ("ent", ent), ("value", value)):
        x = torch.as_tensor(x).detach().double().cpu().reshape(-1)
        assert bool(torch.isfinite(x).all()), n
        out[n] = float(((x - ref[n]).abs() / ref["fwd_scales"][n].clamp_min(1e-300)).max())
    return out


# ------------------------------------------------------------------------------------------------ branch points
def branch_distances(logp, v, rec, clip, norm_adv, vmode):
    """Per sample, in fp64, the distance from every decision one step takes: the ratio from each clip edge (and |ratio - 1| from
    clip, the clip fraction's test); -a * ratio from -a * clamp(ratio) where the ratio is clamped; in value mode 1 |v - v_old|
    from clip and (v - ret)^2 from (v_clipped - ret)^2 where the value is clamped.  Where a decision does not arise: inf."""
    c, lo, hi = f32(clip), f32(1 - clip), f32(1 + clip)
    rec = rec.double()
    old_lp, adv, ret, old_v = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    inf = torch.full_like(logp, float("inf"))
    ratio = (logp - old_lp).exp()
    d_ratio = torch.minimum(torch.minimum((ratio - lo).abs(), (ratio - hi).abs()), ((ratio - 1).abs() - c).abs())
    an = (adv - adv.mean()) / (adv.std() + 1e-8) if norm_adv else adv
    rc = ratio.clamp(lo, hi)
    d_pg = torch.where(rc != ratio, (an * (ratio - rc)).abs(), inf)
    d_dv, d_vmax = inf, inf
    if vmode == O.VLOSS_CLIPPED:
        dv = v - old_v
        d_dv = (dv.abs() - c).abs()
        vcl = old_v + dv.clamp(-c, c)
        d_vmax = torch.where(dv.abs() > c, ((v - ret) ** 2 - (vcl - ret) ** 2).abs(), inf)
    return dict(ratio=d_ratio, pg=d_pg, dv=d_dv, vmax=d_vmax)


def make_records_safe(logp, v, rec_pool, idx, clip, norm_adv, vmode):
    """Move the records (fp32, (B, 4), in place) of the samples that ``idx`` selects until none is within BRANCH_EPS of a branch
    point: old_logp steps 0.02 towards the new log-prob (ratio towards 1, where nothing is clamped), old_v steps 0.01, ret steps
    0.25; re-checked after every move, in fp64, on the fp32 values the kernels will read.  Returns how many records moved.
    Asserts that ZERO samples remain inside the margin: no test excludes a sample."""
    idx = idx.long()
    moved = torch.zeros(rec_pool.shape[0], dtype=torch.bool)
    for _ in range(500):
        rec = rec_pool[idx]
        d = branch_distances(logp, v, rec, clip, norm_adv, vmode)
        bad_lp = (d["ratio"] < BRANCH_EPS) | (d["pg"] < BRANCH_EPS)
        bad_ov, bad_ret = d["dv"] < BRANCH_EPS, d["vmax"] < BRANCH_EPS
        if not bool((bad_lp | bad_ov | bad_ret).any()):
            break
        # a pool row may be selected more than once (an index with repeats): move each row once
        step_lp = torch.zeros(rec_pool.shape[0], dtype=torch.float64)
        step_lp[idx[bad_lp]] = (0.02 * torch.sign(logp - rec[:, 0].double()))[bad_lp]
        rec_pool[:, 0] = (rec_pool[:, 0].double() + step_lp).float()
        rows_ov, rows_ret = torch.unique(idx[bad_ov & ~bad_lp]), torch.unique(idx[bad_ret & ~bad_lp & ~bad_ov])
        rec_pool[rows_ov, 3] += 0.01
        rec_pool[rows_ret, 2] += 0.25
        moved[idx[bad_lp | bad_ov | bad_ret]] = True
    d = branch_distances(logp, v, rec_pool[idx], clip, norm_adv, vmode)
    worst = min(float(x.min()) for x in d.values())
    n_unsafe = int(sum((x < BRANCH_EPS).sum() for x in d.values()))
    assert n_unsafe == 0, f"{n_unsafe} samples within {BRANCH_EPS} of a branch point (closest {worst:.3e})"
    return int(moved.sum())


# ------------------------------------------------------------------------------------------------ cases
# kind: "k7" (2 x 64, D <= 64) or "k7w"; regime: "normal", "scaled" (observations x 1e3, first-layer weights x 1e-3: operands
# whose planes lie many binades apart), "bf16half" (every other observation column exactly representable in bf16: planes
# 1 and 2 of those operands are exactly zero); index: "perm" (distinct rows) or "repeat" (rows drawn with replacement)
Case = collections.namedtuple("Case", "kind hidden layers D A cont M norm_adv vmode regime index packed seed")


def case_id(c):
    return (f"{c.kind}-{c.layers}x{c.hidden}-D{c.D}-A{c.A}-{'gauss' if c.cont else 'cat'}-M{c.M}-"
            f"{'norm' if c.norm_adv else 'raw'}-v{c.vmode}-{c.regime}-{c.index}{'-packed' if c.packed else ''}")


def _mk(kind, hidden, layers, D, A, cont, M, norm_adv, vmode, regime="normal", index="perm", packed=False):
    seed = (hidden * 7 + layers * 131 + D * 17 + A * 29 + M + vmode * 3 + int(norm_adv)) % 100003
    return Case(kind, hidden, layers, D, A, bool(cont), M, bool(norm_adv), vmode, regime, index, bool(packed), seed)


# K7: D over float4 rows and 16-wide k-steps, A over the padded head, M over one tile / a tile plus a row / more tiles than
# workgroups; every (head, value mode, normalisation, regime, index, packed) value appears; the large M once per head
K7_CASES = [
    _mk("k7", 64, 2, 1, 1, True, 1, False, 0), _mk("k7", 64, 2, 3, 2, False, 2, True, 1), _mk("k7", 64, 2, 4, 6, True, 31, True, 1, packed=True),
    _mk("k7", 64, 2, 5, 12, True, 32, False, 2, "bf16half", packed=True), _mk("k7", 64, 2, 15, 16, True, 33, True, 0, "scaled"),
    _mk("k7", 64, 2, 16, 2, False, 63, False, 1, "normal", "repeat"), _mk("k7", 64, 2, 17, 6, True, 65, True, 1, "bf16half", "repeat"),
    _mk("k7", 64, 2, 63, 1, True, 1000, True, 2, "scaled", packed=True), _mk("k7", 64, 2, 64, 6, True, 1000, True, 1),
    _mk("k7", 64, 2, 64, 16, False, 1000, True, 0, "bf16half"), _mk("k7", 64, 2, 64, 12, False, 33, False, 2, "scaled", packed=True),
    _mk("k7", 64, 2, 16, 6, True, 32768 + 17, False, 1, "normal", "repeat"), _mk("k7", 64, 2, 64, 6, True, 131072, True, 1, packed=True),
    _mk("k7", 64, 2, 4, 2, False, 32768 + 17, True, 1),
]
# K7w: the same edges plus D in {65, 100, 127, 128} and hidden over 7 ... 128; ids 1 (hidden <= 64 and D <= 64) and 3 / 2 (wider)
K7W_CASES = [
    _mk("k7w", 7, 1, 3, 1, True, 1, False, 0), _mk("k7w", 32, 2, 5, 2, False, 2, True, 1), _mk("k7w", 64, 3, 15, 6, True, 31, True, 1, packed=True),
    _mk("k7w", 64, 1, 64, 12, True, 65, False, 2, "bf16half", "repeat"), _mk("k7w", 32, 3, 63, 16, False, 1000, True, 0, "scaled"),
    _mk("k7w", 64, 3, 16, 6, True, 32768 + 17, True, 1, "normal", "repeat"),
    _mk("k7w", 65, 1, 1, 1, True, 1, False, 2), _mk("k7w", 65, 2, 17, 2, False, 33, True, 1, "bf16half"), _mk("k7w", 96, 3, 65, 6, True, 63, False, 1, "scaled"),
    _mk("k7w", 100, 2, 100, 12, True, 32, True, 0, packed=True), _mk("k7w", 128, 1, 127, 16, True, 1000, True, 1, "bf16half"),
    _mk("k7w", 128, 3, 128, 6, True, 1000, True, 1, "scaled", "repeat", True), _mk("k7w", 128, 2, 4, 16, False, 65, False, 2, "normal", "repeat"),
    _mk("k7w", 64, 2, 128, 2, False, 1000, True, 1), _mk("k7w", 128, 2, 64, 6, True, 2, True, 2),
    _mk("k7w", 128, 3, 64, 6, True, 32768 + 17, False, 1, "normal", "repeat"), _mk("k7w", 128, 2, 64, 6, True, 131072, True, 1, packed=True),
]
# per-sample forward (minibatches of one sample): 64 samples per shape
FWD_CASES = [
    _mk("k7", 64, 2, 64, 6, True, 64, False, 0), _mk("k7", 64, 2, 17, 16, False, 64, False, 0, "scaled"), _mk("k7", 64, 2, 3, 1, True, 64, False, 0, "bf16half"),
    _mk("k7w", 32, 3, 15, 12, True, 64, False, 0, "bf16half"), _mk("k7w", 64, 1, 63, 2, False, 64, False, 0),
    _mk("k7w", 128, 3, 128, 6, True, 64, False, 0, "scaled"), _mk("k7w", 100, 2, 65, 16, False, 64, False, 0), _mk("k7w", 65, 1, 127, 1, True, 64, False, 0, "bf16half"),
]
HYPER = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5)


def make_policy_sd(hidden, layers, D, A, cont, rs, w1_scale=1.0):
    """Weights from numpy's legacy generator (no LAPACK in the way: the same bits on every machine).  Every layer matters:
    pre-activations O(1), Gaussian means O(0.5), logits O(1), values O(1)."""
    sd = collections.OrderedDict()
    if cont:
        sd["actor_logstd"] = (0.3 * rs.standard_normal((1, A))).astype(np.float32)
    for net, out, head in (("actor", A, 0.5 if cont else 1.0), ("critic", 1, 1.0)):
        dims = [D] + [hidden] * layers + [out]
        for l in range(layers + 1):
            gain = head if l == layers else 1.0
            w = gain * rs.standard_normal((dims[l + 1], dims[l])) / math.sqrt(dims[l])
            if l == 0:
                w = w * w1_scale
            sd[f"{net}.net.{2 * l}.weight"] = w.astype(np.float32)
            sd[f"{net}.net.{2 * l}.bias"] = (0.1 * rs.standard_normal(dims[l + 1])).astype(np.float32)
    return collections.OrderedDict((k, torch.from_numpy(v)) for k, v in sd.items())


def make_obs(B, D, regime, rs):
    obs = rs.standard_normal((B, D)).astype(np.float32)
    if regime == "scaled":
        obs = (obs * np.float32(1e3)).astype(np.float32)
    t = torch.from_numpy(obs)
    if regime == "bf16half":
        t[:, 0::2] = t[:, 0::2].bfloat16().float()
    return t


def build_case(c):
    """Everything a case feeds the kernels, as CPU fp32 tensors, plus the fp64 net: dict(sd, net64, obs (B, D), act, rec (B, 4),
    idx (M,) int32, moved).  The records are margin-safe for the minibatch ``idx`` selects (asserted)."""
    rs = np.random.RandomState(c.seed)
    sd = make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs, 1e-3 if c.regime == "scaled" else 1.0)
    if c.index == "perm":
        B = c.M + 37
        idx = torch.from_numpy(rs.permutation(B)[:c.M].astype(np.int32))
    else:
        B = max(2, c.M // 2 + 1)
        idx = torch.from_numpy(rs.randint(0, B, size=c.M).astype(np.int32))
    obs = make_obs(B, c.D, c.regime, rs)
    act = torch.from_numpy(rs.standard_normal((B, c.A)).astype(np.float32) if c.cont
                           else rs.randint(0, c.A, size=B).astype(np.float32))
    net64 = make_net(sd)
    with torch.no_grad():
        _, lp, _, v = net64.evaluate(obs.double(), act.double() if c.cont else act.long())
    v = v.reshape(-1)
    rec = torch.stack([lp + 0.2 * torch.from_numpy(rs.standard_normal(B)), 2 * torch.from_numpy(rs.standard_normal(B)),
                       v + torch.from_numpy(rs.standard_normal(B)), v + 0.25 * torch.from_numpy(rs.standard_normal(B))], 1).float()
    li = idx.long()
    moved = make_records_safe(lp[li], v[li], rec, idx, HYPER["clip"], c.norm_adv, c.vmode)
    return dict(sd=sd, net64=net64, obs=obs, act=act, rec=rec.contiguous(), idx=idx, moved=moved)


def reference_step(c, data):
    """The fp64 step of a case on its gathered minibatch."""
    li = data["idx"].long()
    return run_step(data["net64"], data["obs"][li].double(), data["act"][li].double(), data["rec"][li].double(),
                    HYPER["clip"], HYPER["ent_coef"], HYPER["vf_coef"], c.norm_adv, c.vmode, scales=True)


def yardstick_step(c, data, device):
    """The same step in plain PyTorch fp32 autograd on ``device`` (no kernel of this project), measured against fp64 on the
    same metrics.  Returns (Y, Y_scalars, per-tensor metrics): Y is the worst tensor's metric; per scalar max(metric, one fp32 ulp
    of the scale), because a mean that torch happens to round exactly must not make the bar zero."""
    ref = data.get("ref") or reference_step(c, data)
    li = data["idx"].long()
    net = make_net(data["sd"], torch.float32, device)
    got = run_step(net, data["obs"][li].to(device), data["act"][li].to(device), data["rec"][li].to(device),
                   HYPER["clip"], HYPER["ent_coef"], HYPER["vf_coef"], c.norm_adv, c.vmode)
    gm = grad_metrics(got["flat"], ref)
    sm = scalar_metrics(got["scalars"], ref)
    return max(gm.values()), {k: max(v, ULP32) for k, v in sm.items()}, gm


def grad_margin(M):
    return MARGIN if M >= TINY_M else MARGIN_TINY_M


def check_step(c, sc, g, ref, Y, Ys, label=""):
    """The bars of one launch: every gradient tensor <= grad_margin(M) * Y, every scalar <= MARGIN_SCALARS * (worst of the nine
    scalars' yardsticks).  Returns (per-tensor metrics, per-scalar metrics, worst tensor ratio, worst scalar ratio) after
    printing them; raises AssertionError naming the tensor / scalar that misses."""
    gm, sm = grad_metrics(g, ref), scalar_metrics(sc, ref)
    Ysc = max(Ys.values())
    worst, ws = max(gm, key=gm.get), max(sm, key=sm.get)
    rg = gm[worst] / Y if Y > 0 else (0.0 if gm[worst] == 0 else float("inf"))
    print(f"\n[{label}] {case_id(c)}: worst tensor {worst} {gm[worst]:.3e} = {rg:.2f} x Y ({Y:.3e}, margin {grad_margin(c.M):g}); "
          f"worst scalar {ws} {sm[ws]:.3e} = {sm[ws] / Ysc:.2f} x Y ({Ysc:.3e}, margin {MARGIN_SCALARS:g})")
    for n, m in gm.items():
        assert m <= grad_margin(c.M) * Y, (label, n, m, Y, m / Y if Y > 0 else float("inf"))
    for n, m in sm.items():
        assert m <= MARGIN_SCALARS * Ysc, (label, n, m, Ysc, m / Ysc)
    return gm, sm, rg, sm[ws] / Ysc


# ------------------------------------------------------------------------------------------------ the rollout step
def act_reference(net64, obs, noise):
    """fp64 rollout step: value; Gaussian head: action = mean + std * noise and its log-prob; Categorical head: the CDF the
    uniform draw is compared with (the sampled index is the number of edges <= the draw, as K8 counts them), the index and
    its log-prob.  Scales as in ``_forward_scales``."""
    saved = {}
    hooks = [m.register_forward_hook((lambda n: lambda _m, i, o: saved.__setitem__(n, (i[0].detach(), o.detach())))(n))
             for n, m in net64.named_modules() if isinstance(m, nn.Linear)]
    with torch.no_grad():
        obs = obs.double()
        v = net64.value(obs)
        mu = net64.actor(obs)
        if net64.continuous:
            a = mu + net64.actor_logstd.exp() * noise.double()
            _, lp, _, _ = net64.evaluate(obs, a)
            cdf = None
        else:
            cdf = torch.softmax(mu, 1).cumsum(1)
            a = (noise.double()[:, None] >= cdf[:, :-1]).sum(1)
            lp = torch.log_softmax(mu, 1).gather(1, a[:, None])[:, 0]
    for h in hooks:
        h.remove()
    sc = _forward_scales(net64, saved, a if net64.continuous else a.double())
    mod = dict(net64.named_modules())[_head(net64, "actor")]
    s_mu = saved[_head(net64, "actor")][0].abs() @ mod.weight.detach().abs().t() + mod.bias.detach().abs()
    s_a = s_mu + (net64.actor_logstd.detach().exp() * noise.double()).abs() if net64.continuous else None
    return dict(value=v, action=a, logp=lp, cdf=cdf, fwd_scales=dict(value=sc["value"], logp=sc["logp"], action=s_a))


def safe_uniform(net64, obs, u):
    """Move the uniform draws (fp32, in place) that lie within BRANCH_EPS of an edge of the fp64 CDF by steps of 1e-3 (wrapping
    inside [0, 1)) until none does; asserts zero remain.  Returns how many moved."""
    with torch.no_grad():
        cdf = torch.softmax(net64.actor(obs.double()), 1).cumsum(1)[:, :-1]
    moved = torch.zeros_like(u, dtype=torch.bool)
    for _ in range(2000):
        bad = ((u.double()[:, None] - cdf).abs() < BRANCH_EPS).any(1)
        if not bool(bad.any()):
            break
        u[bad] = ((u[bad].double() + 1e-3) % 0.999).float()
        moved |= bad
    assert int(((u.double()[:, None] - cdf).abs() < BRANCH_EPS).any(1).sum()) == 0
    return int(moved.sum())


# ------------------------------------------------------------------------------------------------ bf16 x 3 emulation
# csrc/bf16x3.h: a = a0 + a1 + a2 with a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1) (exact); a product is the six plane
# products a0*b0 + (a0*b1 + a1*b0) + (a0*b2 + a2*b0 + a1*b1), each exact, accumulated in fp32.  Here: the chosen plane products
# accumulated in fp64 (exact to 2^-53) and rounded to fp32 once, i.e. the arithmetic the kernels claim at its best.
SIX = frozenset({(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)})
THIRD_ORDER = ((0, 2), (2, 0), (1, 1))
ROLES = ("fwd", "dx", "dw")


def split3(x):
    p0 = x.bfloat16().float()
    r = x - p0
    p1 = r.bfloat16().float()
    p2 = (r - p1).bfloat16().float()
    return p0.double(), p1.double(), p2.double()


def mm3(a, b, prods):
    """(m, k) @ (k, n) from the plane products ``prods`` = {(i, j)}: plane i of ``a`` times plane j of ``b``."""
    pa, pb = split3(a), split3(b)
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
    for i, j in sorted(prods):
        acc += pa[i] @ pb[j]
    return acc.float()


class _Linear3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, prods):
        ctx.save_for_backward(x, w)
        ctx.prods = prods
        return mm3(x, w.t(), prods["fwd"]) + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return mm3(g, w, ctx.prods["dx"]), mm3(g.t(), x, ctx.prods["dw"]), g.sum(0), None


class EmulatedLinear(nn.Module):
    is_linear = True

    def __init__(self, lin, prods):
        super().__init__()
        self.weight, self.bias, self.prods = lin.weight, lin.bias, prods

    def forward(self, x):
        return _Linear3.apply(x, self.weight, self.bias, self.prods)


def make_emulated_net(sd, prods_of):
    """The fp32 CPU net with every Linear's three products (roles fwd / dx / dw) formed by ``mm3``.  ``prods_of(layer, role)``
    returns the plane products of that role; ``layer`` is 0 for the first layer ... ``layers`` for the head, in both nets."""
    net = make_net(sd, torch.float32)
    layers = net_shape(sd)[3]
    for which in ("actor", "critic"):
        seq = getattr(net, which).net
        for l in range(layers + 1):
            seq[2 * l] = EmulatedLinear(seq[2 * l], {r: frozenset(prods_of(l, r)) for r in ROLES})
    return net


class _FastTanh(nn.Module):
    """The forward formula only: its backward is autograd's of the formula, 2 e^{2x} / (e^{2x} + 1)^2 * 2, which is inf / inf = NaN once
    e^{2x} overflows (x > 44.4).  The kernels form tanh' as 1 - t * t from the output, which is clean there; the extremes
    (tests/ref64_extremes.py) therefore use renditions with that backward, and this one serves as their first mutant."""

    def forward(self, x):             # tanh(x) = 1 - 2 / (e^{2x} + 1) (csrc/mlp_common.h): absolute error ~1e-7 everywhere
        return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)


def make_alternative_fp32_net(sd):
    """ANOTHER legitimate fp32 formulation of the step on the CPU: the six-product emulation (exact products, better than fp32) with
    the formulas the kernels' sources use where they differ from torch's -- tanh as 1 - 2 / (e^{2x} + 1), the Gaussian log-prob with
    1 / (std * std) formed once and multiplied in, the Categorical head through max-subtracted exponentials.  Measured against Y
    like a kernel, it shows how far two correct fp32 computations of one case lie apart: the class margins come from it."""
    net = make_emulated_net(sd, lambda l, r: SIX)
    for which in ("actor", "critic"):
        seq = getattr(net, which).net
        for i in range(len(seq)):
            if isinstance(seq[i], nn.Tanh):
                seq[i] = _FastTanh()

    def evaluate(obs, act):
        mu, v = net.actor(obs), net.critic(obs)
        if net.continuous:
            ls = net.actor_logstd.expand_as(mu)
            sd_ = torch.exp(ls)
            z = act - mu
            return act, ((-(z * z) * (0.5 * (1.0 / (sd_ * sd_))) - ls) - _HALF_LOG_2PI).sum(1), ((0.5 + _HALF_LOG_2PI) + ls).sum(1), v
        mx = mu.max(1, keepdim=True).values
        lp = mu - (mx + torch.log(torch.exp(mu - mx).sum(1, keepdim=True)))
        return act, lp.gather(1, act[:, None])[:, 0], -(torch.exp(lp) * lp).sum(1), v
    net.evaluate = evaluate
    return net


# ------------------------------------------------------------------------------------------------ launching the kernels (GPU)
Kernel = collections.namedtuple("Kernel", "name env k7_variant k7w_id")


def kernels_for(c):
    """Every build of the step a case's shape can be dispatched to, with the knobs that select it."""
    if c.kind == "k7":
        return [Kernel("K7:k_mlp_step3", {"AURPPO_K7_VARIANT": "3"}, 3, None), Kernel("K7:k_mlp_step2", {"AURPPO_K7_VARIANT": "2"}, 2, None)]
    if c.hidden <= 64 and c.D <= 64:
        return [Kernel("K7w:id1:k_mlpw_step<L,true>", {"AURPPO_K7W_VARIANT": "3"}, None, 1)]
    return [Kernel("K7w:id3:k_mlpw3_step<L>", {"AURPPO_K7W_VARIANT": "3"}, None, 3),
            Kernel("K7w:id2:k_mlpw_step<L,false>", {"AURPPO_K7W_VARIANT": "2"}, None, 2)]


def select_kernel(c, k, static, setenv):
    """Set the knobs (``setenv(name, value)``: monkeypatch.setenv in tests), make the library read them, and ASSERT which kernel
    this shape is dispatched to.  Returns the kernel's label."""
    from aur_ppo_amd import hip_ops as H
    for name, val in k.env.items():
        setenv(name, val)
    setenv("AURPPO_STATIC_TILES", str(static))
    H.reload_knobs()
    if k.k7_variant is not None:
        assert H.k7_variant() == k.k7_variant, (H.k7_variant(), k)
        return f"{k.name} (aurppo_k7_variant {H.k7_variant()})"
    assert H.k7w_kernel(c.hidden, c.D) == k.k7w_id, (H.k7w_kernel(c.hidden, c.D), k)
    return f"{k.name} (aurppo_k7w_kernel {H.k7w_kernel(c.hidden, c.D)}: {H.k7w_kernel_name(c.hidden, c.D, c.layers)})"


def gpu_policy(c, sd):
    """The project's actor_critic with the case's weights on the GPU, its flat bucket and its kernel layout."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    pol.load_state_dict(sd)
    pol = pol.cuda()
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layout(pol, bucket)
    assert lay is not None and lay["wide"] == (c.kind == "k7w") and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (c.D, c.A, c.hidden, c.layers)
    assert [n for n, _ in pol.named_parameters()] == param_names(make_net(sd)), "FlatBucket order"
    return pol, bucket, lay


def gpu_inputs(c, data):
    """obs, actions, records (packed into 64-byte rows if the case says so) and index on the GPU, as the step takes them."""
    from aur_ppo_amd import hip_ops as H
    obs, act, rec, idx = (data[k].cuda().contiguous() for k in ("obs", "act", "rec", "idx"))
    if c.packed:
        return obs, None, H.pack_records(rec, act.reshape(rec.shape[0], -1)), idx
    return obs, act, rec, idx


def kernel_step(c, data, pol_bucket_lay, norm_adv=None, vmode=None, idx=None, vf_coef=None):
    """One launch of the fused step through ``hip_ops.mlp_ppo_step``; returns (scalars, flat gradient) on the GPU."""
    from aur_ppo_amd import hip_ops as H
    _pol, bucket, lay = pol_bucket_lay
    obs, act, rec, idx0 = data["gpu"]
    g_out = torch.full_like(bucket.flat_grad, float("nan"))
    sc = H.mlp_ppo_step(obs, act, rec, idx0 if idx is None else idx, bucket.flat_param, lay, g_out, HYPER["clip"], HYPER["ent_coef"],
                        HYPER["vf_coef"] if vf_coef is None else vf_coef, c.norm_adv if norm_adv is None else norm_adv,
                        c.vmode if vmode is None else vmode)
    return sc, g_out[:lay["n_params"]]
