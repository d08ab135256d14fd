"""Routing-pinned fp64 reference of the robot policy's PPO step (``robot_actor_critic(equivariant=False)``: two ``base_encoder``s, the
Gaussian head and the critic's Linear-ReLU-Linear, under the loss of src/robot_ppo.py:370-400), the metric its gradients are judged on,
and what records / compares the ReLU and max-pool decisions a path took.  A plain helper module (no tests in it); DESIGN 2.5 derives the
bars, tests/test_robot_ref64_host.py re-derives them on the CPU.

Why pinned: ReLU and max-pool are decisions.  An fp32 and an fp64 evaluation legitimately part ways on a few near-ties, and one flipped
window moves a gradient element by a whole term.  So the reference is the same network with every decision GIVEN (``routing``: per
pooled block a window index 0..3 in the kernels' order ``u = 2 * (row & 1) + (col & 1)``, 4 = dead; per bare ReLU a 0 / 1 mask): given
the routing the net is smooth and fp64 is exact.  ``check_routing`` holds the decisions themselves to the fp64 ones wherever those are
not near-ties.

The metric: DESIGN 2.1's sums of |terms| (for a convolution's dW the weight gradient of conv2d(|x|, .) against |dz|), taken PER TENSOR:
max |g - g64| over the tensor's largest sum of |terms|.  Element by element the metric is not usable for this net -- at 32 samples a dW
element of a late layer is often one or two terms dz * x, each of which came out of a cancelling sum, and plain fp32 torch itself sits at
1.6 ... 880 on it depending on the seed -- so the per-element figure is printed beside the asserted one, not asserted.

What is here
  * ``forward_pinned`` / ``step``: the net and the loss in torch ops, in the dtype asked for: float64 is the REFERENCE, float32 the
    YARDSTICK Y (plain fp32 torch on the same routing, case and metric); ``split_first`` is a second correct fp32 formulation (the first
    convolution in the split form the product uses), ``conv_of`` replaces chosen convolutions (the bf16x3 mutants of the host test).
  * ``grad_metrics`` / ``forward_metrics`` / ``yardstick`` / ``check``: the bars.
  * ``capture_routing`` / ``check_routing``: the decisions of the path under test, and their comparison with the fp64 ones.
  * ``make_policy`` / ``make_buffers`` / ``make_case``: weights from ``torch.manual_seed``, data from tests/test_robot_gpu.py's generator,
    the records moved clear of the loss's own branches.
"""
from __future__ import annotations

import collections
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from oracle import ppo_oracle as O
from tests import ref64_loss as RL
from tests.ref64 import MARGIN, MARGIN_SCALARS, SCALAR_NAMES, SIX, THIRD_ORDER, ULP32, f32, scalar_metrics, split3  # noqa: F401

TAU = 1e-5                 # a decision whose fp64 margin is below TAU x (sum |x||w| + |b|) is a near-tie: the reference follows the path there
NEAR_TIE_CAP = 5e-3        # share of a layer's decisions that may be near-ties (a condition on the inputs: the reference alone is at <= 0.13 %)
HYPER = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5)        # tests/test_robot_gpu.py's configuration
SHAPES = ((1, 128), (3, 84))
M = 32                     # the minibatch of tests/test_robot_gpu.py: the last convolution's dW elements still sum 32 terms
# Bars: metric <= margin * Y.  A second correct fp32 formulation against Y (never a kernel), 60 seeds x both shapes
# (tools/robot_fp64_table.py --margins; tests/test_robot_ref64_host.py re-measures three seeds): worst ratio 3.46 for the gradient tensors
# (Y: torch's measured figure per tensor, see ``yardstick``), 2.11 for log-prob / value, 1.52 for the scalars.  A class whose worst ratio
# is below 2 takes ref64's margin (the scalars: 16); the others the smallest power of two >= 1.25 x the worst ratio: 8 and 4.
MARGIN_GRADS, MARGIN_FWD, MARGIN_SCALARS_ROBOT = 8.0, 4.0, MARGIN_SCALARS
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ the net
def encoder_layers(sd, net):
    """[(index in base_encoder.conv, padding, decision)] of one encoder: 128 x 128 (src/nets/base_cnns.py:20-54) or the 84 x 84 variant."""
    head = [(0, 1, "pool"), (3, 1, "pool"), (6, 1, "pool"), (9, 1, "pool")]
    if f"{net}.conv.conv.17.weight" in sd:
        return head + [(12, 1, "relu"), (14, 0, "pool"), (17, 0, "relu")]
    return head + [(12, 0, "relu"), (14, 0, "relu")]


def n_decisions(sd):
    """Decisions of one ``evaluate`` in network order: the actor's encoder, the critic's encoder, the critic head's ReLU."""
    return len(encoder_layers(sd, "actor")) + len(encoder_layers(sd, "critic")) + 1


def param_names(sd):
    return ["actor_logstd"] + [k for k in sd if k.startswith(("actor.", "critic."))]


def windows(z):
    """(B, C, H, W) -> (B, C, H // 2, W // 2, 4): the 2 x 2 windows of MaxPool2d(2) (an odd last row / column is dropped), u = 2 * row + col."""
    B, C, H, W = z.shape
    Ho, Wo = H // 2, W // 2
    return z[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def pool_decision(wz):
    """The first maximum of each window (torch's scan order, K9's and K10's), 4 where it is not positive (ReLU kills the window)."""
    m, k = wz[..., 0], torch.zeros(wz.shape[:-1], dtype=torch.long, device=wz.device)
    for u in range(1, 4):
        up = wz[..., u] > m
        m, k = torch.where(up, wz[..., u], m), torch.where(up, torch.full_like(k, u), k)
    return torch.where(m > 0, k, torch.full_like(k, 4))


def cat_input(state, obs):
    """src/models/robot_actor_critic.py:58-59: the gripper state tiled to a plane, concatenated as the last input channel."""
    return torch.cat([obs, state.reshape(-1, 1, 1, 1).to(obs.dtype).expand(-1, 1, obs.shape[2], obs.shape[3])], dim=1)


def forward_pinned(net, state, obs, actions, routing=None, dtype=torch.float64, device="cpu", split_first=False, conv_of=None):
    """``evaluate(state, obs, actions)`` of the state dict ``net`` with every ReLU / pool decision taken from ``routing`` (a list in
    network order; None: the run's own decisions, which are returned).  Returns dict(logp, ent, value (per sample), layers (per
    convolution / Linear: name, op, pad, kind, x, z with ``retain_grad``), routing, params (the leaves the gradients land on)).
    ``split_first``: the first convolution as ``conv(obs, w[:, :C]) + state * conv(ones, w[:, C:])``, then ``+ bias``
    (base_encoder.forward_split's association).  ``conv_of``: {layer name: fn(x, w, pad)} replacing that convolution (bias added here)."""
    P = collections.OrderedDict((k, net[k].detach().to(dtype=dtype, device=device).clone().requires_grad_()) for k in param_names(net))
    state, obs, actions = (t.detach().to(dtype=dtype, device=device) for t in (state, obs, actions))
    route = None if routing is None else list(routing)
    used, layers = [], []

    def decide(z, kind):
        if kind == "pool":
            wz = windows(z)
            k = pool_decision(wz.detach()) if route is None else route.pop(0).to(device=device, dtype=torch.long)
            assert k.shape == wz.shape[:-1], (k.shape, wz.shape)
            used.append(k)
            return wz.gather(-1, k.clamp(max=3).unsqueeze(-1)).squeeze(-1) * (k < 4).to(dtype)
        m = (z.detach() > 0) if route is None else route.pop(0).to(device=device, dtype=torch.bool)
        assert m.shape == z.shape, (m.shape, z.shape)
        used.append(m)
        return z * m.to(dtype)

    def layer(name, op, pad, kind, x, z):
        if z.requires_grad:
            z.retain_grad()
        layers.append(dict(name=name, op=op, pad=pad, kind=kind, x=x.detach(), z=z))
        return z if kind is None else decide(z, kind)

    def encoder(which):
        x = cat_input(state, obs)
        for i, pad, kind in encoder_layers(net, which):
            name = f"{which}.conv.conv.{i}"
            w, b = P[name + ".weight"], P[name + ".bias"]
            if i == 0 and split_first:
                c = obs.shape[1]
                ones = torch.ones((1, 1) + tuple(obs.shape[2:]), dtype=dtype, device=device)
                z = F.conv2d(obs, w[:, :c], None, padding=pad)
                z = z + state.reshape(-1, 1, 1, 1) * F.conv2d(ones, w[:, c:c + 1], None, padding=pad) + b.reshape(1, -1, 1, 1)
            elif conv_of and name in conv_of:
                z = conv_of[name](x, w, pad) + b.reshape(1, -1, 1, 1)
            else:
                z = F.conv2d(x, w, b, padding=pad)
            x = layer(name, "conv", pad, kind, x, z)
        return x.flatten(1)

    def linear(name, kind, x):
        return layer(name, "linear", 0, kind, x, F.linear(x, P[name + ".weight"], P[name + ".bias"]))

    mean = linear("actor.mean_linear", None, encoder("actor"))
    h = linear("critic.critic.0", "relu", encoder("critic"))
    value = linear("critic.critic.2", None, h).reshape(-1)
    assert route is None or not route, "routing has more entries than the net has decisions"
    logstd = P["actor_logstd"].expand_as(mean)
    std = torch.exp(logstd)
    d = actions - mean                                           # robot_actor_critic.evaluate, term for term
    logp = (-(d * d) / (2 * std * std) - logstd - _HALF_LOG_2PI).sum(1)
    ent = (0.5 + _HALF_LOG_2PI + logstd).sum(1)
    return dict(logp=logp, ent=ent, value=value, mean=mean, layers=layers, routing=used, params=P)


def preact_scales(out):
    """Per decision, in network order: (kind, z, sum |x||w| + |b| behind every element of z) of a ``forward_pinned`` result."""
    res, P = [], out["params"]
    with torch.no_grad():
        for L in out["layers"]:
            if L["kind"] is None:
                continue
            w, b = P[L["name"] + ".weight"].abs(), P[L["name"] + ".bias"].abs()
            s = F.conv2d(L["x"].abs(), w, b, padding=L["pad"]) if L["op"] == "conv" else F.linear(L["x"].abs(), w, b)
            res.append((L["kind"], L["z"].detach(), s))
    return res


# ------------------------------------------------------------------------------------------------ the step
def step(net, case, routing=None, vmode=O.VLOSS_CLIPPED, dtype=torch.float64, device="cpu", norm_adv=True, hyper=HYPER, scales=False,
         **fw):
    """One minibatch step on ``case`` (dict: state (M,), obs (M, C, S, S), act (M, 5), rec (M, 4) = {old_logp, adv, ret, old_v}):
    ``forward_pinned``, ``ref64_loss.run_terms`` (ref64.loss_terms with the fp32 roundings of the hyper-parameters) on its log-prob /
    entropy / value, and autograd through the net.  Returns dict(scalars (9), scalar_scales, names, grads {name: tensor}, logp, ent,
    value, routing, out) and with ``scales`` (the fp64 run) grad_scales {name: tensor}, fwd_scales {logp, value} and ``decisions``
    (``preact_scales``)."""
    out = forward_pinned(net, case["state"], case["obs"], case["act"], routing, dtype, device, **fw)
    x = dict(newlogp=out["logp"].detach(), newv=out["value"].detach(), entropy=out["ent"].detach(), rec=case["rec"].to(device))
    t = RL.run_terms(x, hyper, norm_adv, vmode, dtype)
    torch.autograd.backward([out["logp"], out["ent"], out["value"]], [t["g_newlogp"], t["g_entropy"], t["g_newv"]])
    P = out["params"]
    grads = collections.OrderedDict((n, torch.zeros_like(p) if p.grad is None else p.grad.detach()) for n, p in P.items())
    res = dict(scalars=t["scalars"], scalar_scales=t["scalar_scales"], names=list(P), grads=grads, logp=out["logp"].detach(),
               ent=out["ent"].detach(), value=out["value"].detach(), routing=out["routing"], out=out)
    if not scales:
        return res
    Mb = case["state"].shape[0]
    gs, g2 = collections.OrderedDict(), {}          # g2: the sums of the SQUARED terms, for ``grad_floors``
    with torch.no_grad():
        std = P["actor_logstd"].detach().exp()
        zz = (case["act"].to(dtype=dtype, device=device) - out["mean"].detach()) / std
        # per-sample term of d loss / d logstd_j: g_logp_s * (z_sj^2 - 1) from the log-prob, -ent_coef / M from the entropy
        tl = t["g_newlogp"][:, None] * (zz * zz - 1) - f32(hyper["ent_coef"]) / Mb
        gs["actor_logstd"], g2["actor_logstd"] = tl.abs().sum(0, keepdim=True), (tl * tl).sum(0, keepdim=True)
    for L in out["layers"]:
        dz, xa = L["z"].grad.abs(), L["x"].abs()
        if L["op"] == "conv":
            # the weight gradient of conv2d(|x|, .) against |dz| (tests/test_conv_gpu.py::wgrad64)
            wd = torch.zeros_like(P[L["name"] + ".weight"]).requires_grad_()
            F.conv2d(xa, wd, None, padding=L["pad"]).backward(dz)
            gs[L["name"] + ".weight"], gs[L["name"] + ".bias"] = wd.grad, dz.sum((0, 2, 3))
            w2 = torch.zeros_like(wd).requires_grad_()
            F.conv2d(xa * xa, w2, None, padding=L["pad"]).backward(dz * dz)
            g2[L["name"] + ".weight"], g2[L["name"] + ".bias"] = w2.grad, (dz * dz).sum((0, 2, 3))
        else:
            gs[L["name"] + ".weight"], gs[L["name"] + ".bias"] = dz.t() @ xa, dz.sum(0)
            g2[L["name"] + ".weight"], g2[L["name"] + ".bias"] = (dz * dz).t() @ (xa * xa), (dz * dz).sum(0)
    by = {L["name"]: L for L in out["layers"]}
    with torch.no_grad():
        hs = lambda n: F.linear(by[n]["x"].abs(), P[n + ".weight"].abs(), P[n + ".bias"].abs())        # noqa: E731
        logstd = P["actor_logstd"].detach().expand_as(zz)
        s_lp = ((zz / std).abs() * hs("actor.mean_linear")).sum(1) + (0.5 * zz * zz + logstd.abs() + _HALF_LOG_2PI).sum(1)
        # what ANY fp32 computation loses on a tensor's largest element: each of its terms t rounded once, 2^-24 rms(t) sqrt(n) over
        # sum |t| = 2^-24 / sqrt(n_eff), n_eff = (sum |t|)^2 / sum t^2 -- the floor of that tensor's yardstick
        floors = collections.OrderedDict()
        for n in P:
            e = int(gs[n].reshape(-1).argmax())
            S, S2 = float(gs[n].reshape(-1)[e]), float(g2[n].reshape(-1)[e])
            floors[n] = ULP32 * math.sqrt(S2) / S if S > 0 else ULP32
        res.update(grad_floors=floors)
        res.update(grad_scales=collections.OrderedDict((n, gs[n]) for n in P), fwd_scales=dict(logp=s_lp, value=hs("critic.critic.2").reshape(-1)),
                   decisions=preact_scales(out))
    return res


# ------------------------------------------------------------------------------------------------ metrics and bars
def _over(err, S):
    """max of err / S; where S is 0 (no term reaches the element) the error must be 0."""
    m = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(m.max())


def grad_metrics(grads, ref, per_element=False):
    """{parameter: max over its elements of |g - g64| / max S}; ``per_element``: of |g - g64| / S element by element.
    ``grads``: {name: tensor} (any device / dtype)."""
    out = collections.OrderedDict()
    for n in ref["names"]:
        g = torch.as_tensor(grads[n]).detach().double().cpu().reshape(ref["grads"][n].shape)
        assert bool(torch.isfinite(g).all()), f"{n}: non-finite gradient"
        S = ref["grad_scales"][n]
        out[n] = _over((g - ref["grads"][n]).abs(), S if per_element else S.max().expand_as(S))
    return out


def forward_metrics(logp, value, ref):
    out = collections.OrderedDict()
    for n, x in (("logp", logp), ("value", value)):
        x = torch.as_tensor(x).detach().double().cpu().reshape(-1)
        assert bool(torch.isfinite(x).all()), n
        out[n] = _over((x - ref[n]).abs(), ref["fwd_scales"][n])
    return out


def all_metrics(got, ref):
    """(gradient, forward, scalar) metrics of a ``step``-shaped result (grads, logp, value, scalars; a missing part is skipped)."""
    return (grad_metrics(got["grads"], ref) if "grads" in got else {}, forward_metrics(got["logp"], got["value"], ref) if "logp" in got else {},
            scalar_metrics(got["scalars"], ref) if "scalars" in got else {})


def yardstick(net, case, ref, vmode, device="cpu", **kw):
    """Y: the same routing-pinned step in plain fp32 torch on ``device`` against ``ref`` on the same metrics.  A gradient tensor's Y is
    torch's MEASURED figure, at least ``grad_floors`` (2^-24 / sqrt(n_eff) of the tensor's largest element: what rounding every term once
    costs -- 1e-10 ... 5e-8 here, far below an ulp for the long sums of the first blocks); forward values and scalars at least one ulp.  Returns dict(grads: {tensor: Y},
    fwd: {logp, value}, scalars: the worst of the nine, per_element: the per-element metric of every tensor, got)."""
    got = step(net, case, ref["routing"], vmode, torch.float32, device, **kw)
    gm, fm, sm = all_metrics(got, ref)
    return dict(grads={n: max(v, ref["grad_floors"][n]) for n, v in gm.items()}, fwd={n: max(v, ULP32) for n, v in fm.items()},
                scalars=max(max(v, ULP32) for v in sm.values()), per_element=grad_metrics(got["grads"], ref, per_element=True), got=got)


def ratios(got, ref, Y):
    """({class: worst metric / Y}, gradient, forward and scalar metrics) of a result."""
    gm, fm, sm = all_metrics(got, ref)
    r = collections.OrderedDict()
    if gm:
        r["grads"] = max(gm[n] / Y["grads"][n] for n in gm)
    if fm:
        r["fwd"] = max(fm[n] / Y["fwd"][n] for n in fm)
    if sm:
        r["scalars"] = max(sm.values()) / Y["scalars"]
    return r, gm, fm, sm


def check(got, ref, Y, label=""):
    """The bars of one result: every gradient tensor <= MARGIN_GRADS * its Y, log-prob and value <= MARGIN_FWD * their Y, every scalar
    <= MARGIN_SCALARS_ROBOT * Y.  Prints metric, Y and ratio per tensor (and the per-element figures of both beside them), then asserts."""
    r, gm, fm, sm = ratios(got, ref, Y)
    print(f"\n[{label}] worst ratios " + "  ".join(f"{k} {v:.2f}" for k, v in r.items())
          + f"   (margins {MARGIN_GRADS:g} / {MARGIN_FWD:g} / {MARGIN_SCALARS_ROBOT:g})")
    pe = grad_metrics(got["grads"], ref, per_element=True) if gm else {}
    for n, m in gm.items():
        print(f"    {n:28s} {m:10.3e}  Y {Y['grads'][n]:10.3e}  = {m / Y['grads'][n]:5.2f} x Y     per element {pe[n]:10.3e}  Y {Y['per_element'][n]:10.3e}")
    for n, m in fm.items():
        print(f"    {n:28s} {m:10.3e}  Y {Y['fwd'][n]:10.3e}  = {m / Y['fwd'][n]:5.2f} x Y")
    if sm:
        ws = max(sm, key=sm.get)
        print(f"    scalars: worst {ws:15s} {sm[ws]:10.3e}  Y {Y['scalars']:10.3e}  = {sm[ws] / Y['scalars']:5.2f} x Y")
    for n, m in gm.items():
        assert m <= MARGIN_GRADS * Y["grads"][n], (label, n, m, Y["grads"][n], m / Y["grads"][n])
    for n, m in fm.items():
        assert m <= MARGIN_FWD * Y["fwd"][n], (label, n, m, Y["fwd"][n], m / Y["fwd"][n])
    for n, m in sm.items():
        assert m <= MARGIN_SCALARS_ROBOT * Y["scalars"], (label, n, m, Y["scalars"], m / Y["scalars"])
    return r


# ------------------------------------------------------------------------------------------------ routing
@contextlib.contextmanager
def capture_routing(policy):
    """Record the decisions every ``policy.evaluate`` inside the block takes, in network order.  K9 / K10 blocks: the byte mask the
    kernel wrote (saved on the autograd node; ``hip_ops.bias_relu_pool2`` / ``first_block`` are wrapped, so evaluate with grad enabled).
    Modules that run as nn.ReLU / nn.MaxPool2d: forward hooks (``out > 0``; the pool's argmax as a window index, replacing the
    record of the ReLU in front of it).  Yields (records, counts of K9 / K9 with the plane operands / K10 calls)."""
    from aur_ppo_amd import hip_ops as H
    rec, counts = [], collections.Counter()
    real = dict(bias_relu_pool2=H.bias_relu_pool2, first_block=H.first_block)

    def mask_of(y):
        return next(t for t in y.grad_fn.saved_tensors if t is not None and t.dtype == torch.uint8).clone()

    def brp(x, bias=None, scale=None, plane=None):
        y = real["bias_relu_pool2"](x, bias, scale, plane)
        rec.append(mask_of(y))
        counts["K9"] += 1
        counts["K9_plane"] += int(plane is not None and scale is not None)
        return y

    def fb(obs, state, weight, bias):
        y = real["first_block"](obs, state, weight, bias)
        rec.append(mask_of(y))
        counts["K10"] += 1
        return y

    def relu_hook(_m, _i, out):
        rec.append(out.detach() > 0)
        counts["relu"] += 1

    def pool_hook(_m, inp, _o):
        x = inp[0].detach()                                   # the ReLU's output
        vals, idx = F.max_pool2d(x, 2, return_indices=True)
        u = 2 * ((idx // x.shape[3]) % 2) + (idx % x.shape[3]) % 2
        rec[-1] = torch.where(vals > 0, u, torch.full_like(u, 4))
        counts["pool"] += 1

    hooks = [m.register_forward_hook(relu_hook if isinstance(m, nn.ReLU) else pool_hook)
             for m in policy.modules() if isinstance(m, (nn.ReLU, nn.MaxPool2d))]
    H.bias_relu_pool2, H.first_block = brp, fb
    try:
        yield rec, counts
    finally:
        H.bias_relu_pool2, H.first_block = real["bias_relu_pool2"], real["first_block"]
        for h in hooks:
            h.remove()


def decision_margins(kind, z, scale):
    """(fp64 decision, margin / scale) per decision.  Pooled window: top value minus runner-up, or top value against 0 when that is
    smaller, over the largest of the window's four scales; bare ReLU: |z| over its scale."""
    if kind == "relu":
        return z > 0, z.abs() / scale.clamp_min(1e-300)
    wz, ws = windows(z), windows(scale).max(-1).values
    top2 = wz.topk(2, dim=-1).values
    return pool_decision(wz), torch.minimum(top2[..., 0] - top2[..., 1], top2[..., 0].abs()) / ws.clamp_min(1e-300)


def check_routing(routing, decisions, tau=TAU, label=""):
    """``routing``: what a path decided; ``decisions``: ``step(..., scales=True)["decisions"]`` of the fp64 run pinned to it.  Every
    recorded decision must EQUAL the fp64 one wherever the fp64 margin is at least ``tau`` x the pre-activation's scale (asserted:
    zero disagreements outside the near-tie set), and at most NEAR_TIE_CAP of a layer's decisions may be near-ties (asserted).
    Returns per layer (near-tie share, disagreements inside the near-tie set)."""
    assert len(routing) == len(decisions), (len(routing), len(decisions))
    out = []
    for i, (r, (kind, z, s)) in enumerate(zip(routing, decisions)):
        d64, mg = decision_margins(kind, z, s)
        r = r.cpu().to(d64.dtype)
        assert r.shape == d64.shape, (i, r.shape, d64.shape)
        near = mg < tau
        differ = r != d64
        n_out = int((differ & ~near).sum())
        assert n_out == 0, f"{label} decision layer {i} ({kind}): {n_out} decisions differ from fp64 at a margin >= {tau:g} of the scale"
        share = float(near.double().mean())
        assert share <= NEAR_TIE_CAP, f"{label} decision layer {i} ({kind}): near-tie share {share:.4f} (a property of the inputs: change the seed)"
        out.append((share, int((differ & near).sum())))
    return out


# ------------------------------------------------------------------------------------------------ cases
def make_policy(C, S, seed=2):
    from aur_ppo_amd.robot_actor_critic import robot_actor_critic
    torch.manual_seed(seed)
    return robot_actor_critic(torch.device("cpu"), False, obs_shape=(C, S, S))


def make_buffers(cpu, C, S, gen_seed=9, T=8, N=8):
    """tests/test_robot_gpu.py's data generator: the (T, N) rollout buffers, with log-probs / values from ``cpu``'s fp32 evaluate, and the
    bootstrap state / observation."""
    g = torch.Generator().manual_seed(gen_seed)
    buf = dict(states=(torch.rand(T, N, generator=g) < 0.5).float(), observations=torch.rand(T, N, C, S, S, generator=g),
               actions=0.3 * torch.randn(T, N, 5, generator=g), true_actions=torch.zeros(T, N, 5),
               rewards=(torch.rand(T, N, generator=g) < 0.3).float(), terminals=(torch.rand(T, N, generator=g) < 0.1).float())
    with torch.no_grad():
        _, _, lp, _, v = cpu.evaluate(buf["states"].view(-1), buf["observations"].view(-1, C, S, S), buf["actions"].view(-1, 5))
    buf["log_probs"] = (lp.view(T, N) + 0.05 * torch.randn(T, N, generator=g))
    buf["values"] = v.view(T, N).clone()
    next_state, next_obs = (torch.rand(N, generator=g) < 0.5).float(), torch.rand(N, C, S, S, generator=g)
    return buf, next_state, next_obs


def flat_buffers(cpu, buf, next_state, next_obs, C, S):
    """The tuple of ``torch_buffer.flatten`` with the oracle's skip-last GAE (src/robot_ppo.py:224-244) on the CPU bootstrap value."""
    with torch.no_grad():
        nv = cpu.value(next_state, next_obs).flatten()
    ret, adv = O.gae(buf["rewards"].numpy(), buf["values"].numpy(), buf["terminals"].numpy(), nv.numpy(), np.zeros(nv.numel(), np.float32),
                     0.99, 0.95, O.GAE_MODE_SKIP_LAST)
    return (buf["states"].view(-1), buf["observations"].view(-1, C, S, S), buf["log_probs"].reshape(-1), buf["actions"].view(-1, 5),
            torch.from_numpy(adv).reshape(-1), torch.from_numpy(ret).reshape(-1), buf["values"].reshape(-1), buf["true_actions"].view(-1, 5))


def first_minibatch(B, seed=1, Mb=M):
    """``np.random.RandomState(seed).shuffle``'s first ``Mb`` indices: optimizer step 1 of the update (K2 is bit-exact with it)."""
    idx = np.arange(B)
    np.random.RandomState(seed).shuffle(idx)
    return torch.from_numpy(idx[:Mb].copy()).long()


def make_records_safe(net, case, hyper=HYPER):
    """Move old_logp / old_v / ret of ``case["rec"]`` (in place) clear of the loss's own branches (``ref64_loss.make_safe``: both
    normalisations, every value mode) against the fp64 forward values of the net's own routing; asserts none left.  Returns how many moved."""
    with torch.no_grad():
        out = forward_pinned(net, case["state"], case["obs"], case["act"])
    return RL.make_safe(dict(newlogp=out["logp"].detach(), newv=out["value"].detach(), rec=case["rec"]), hyper["clip"])


_CASES = {}


def make_case(C, S, seed=2):
    """(state dict, case) of one committed case: weights from ``torch.manual_seed(seed)``, data from the generator above (seed + 7: 9
    for the committed seed 2), the first minibatch of 32 of the 64 samples, records safe.  Cached: leave it unchanged."""
    key = (C, S, seed)
    if key not in _CASES:
        cpu = make_policy(C, S, seed)
        buf, ns, no = make_buffers(cpu, C, S, seed + 7)
        st, ob, lp, ac, adv, ret, val, _ = flat_buffers(cpu, buf, ns, no, C, S)
        mb = first_minibatch(st.shape[0])
        sd = collections.OrderedDict((k, v.detach().clone()) for k, v in cpu.state_dict().items())
        case = dict(state=st[mb].clone(), obs=ob[mb].clone(), act=ac[mb].clone(),
                    rec=torch.stack([lp[mb], adv[mb], ret[mb], val[mb]], 1).float().contiguous())
        case["moved"] = make_records_safe(sd, case)
        _CASES[key] = (sd, case)
    return _CASES[key]


_REFS = {}


def routing_key(routing):
    return hash(tuple(r.cpu().to(torch.uint8).numpy().tobytes() for r in routing))


def reference(key, net, case, routing, vmode, hyper=HYPER):
    """The fp64 step of a (case key, routing, value mode), computed once."""
    k = (key, None if routing is None else routing_key(routing), vmode)
    if k not in _REFS:
        _REFS[k] = step(net, case, routing, vmode, torch.float64, "cpu", hyper=hyper, scales=True)
    return _REFS[k]


# ------------------------------------------------------------------------------------------------ bf16 x 3 convolution (the mutants)
def _planes(t):
    return split3(t.float())


class _Conv3(torch.autograd.Function):
    """conv2d from the plane products of csrc/bf16x3.h (ref64.split3's rounding), one set per role: convolution is bilinear, so each
    role is a sum of plane convolutions, accumulated in fp64 and rounded to fp32 once."""

    @staticmethod
    def forward(ctx, x, w, pad, prods):
        ctx.save_for_backward(x, w)
        ctx.pad, ctx.prods = pad, prods
        px, pw = _planes(x), _planes(w)
        return sum(F.conv2d(px[i], pw[j], None, padding=pad) for i, j in sorted(prods["fwd"])).float()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        pg, px, pw = _planes(g), _planes(x), _planes(w)
        dx = sum(torch.nn.grad.conv2d_input(x.shape, pw[j], pg[i], padding=ctx.pad) for i, j in sorted(ctx.prods["dx"])).float()
        dw = sum(torch.nn.grad.conv2d_weight(px[j], w.shape, pg[i], padding=ctx.pad) for i, j in sorted(ctx.prods["dw"])).float()
        return dx, dw, None, None


def conv3(prods):
    """fn(x, w, pad) for ``forward_pinned(conv_of=...)``; ``prods``: {"fwd" / "dx" / "dw": set of (plane of the first operand, plane of
    the second)}, first operand x / dz / dz, second w / w / x."""
    return lambda x, w, pad: _Conv3.apply(x, w, pad, prods)


# ------------------------------------------------------------------------------------------------ the paths under test (GPU)
PATHS = ("product", "hand_written_convolutions", "k9_with_the_plane")


def gpu_policy(sd, C, S):
    from aur_ppo_amd.robot_actor_critic import robot_actor_critic
    pol = robot_actor_critic(torch.device("cuda"), False, obs_shape=(C, S, S))
    pol.load_state_dict(sd)
    return pol.cuda()


def select_path(path, pol, setattr_, setenv):
    """Select one of PATHS on ``pol`` (``setattr_(obj, name, value)`` / ``setenv(name, value)``: monkeypatch's in tests) and wrap the
    hand-written convolutions with call counters.  Returns the Counter (K11 / K12 calls)."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.base_cnns import base_encoder
    assert path in PATHS, path
    calls = collections.Counter()
    real_conv, real_wgrad = H.conv3x3, H.conv3x3_wgrad
    setattr_(H, "conv3x3", lambda x, w, p: (calls.update(K11=1), real_conv(x, w, p))[1])
    setattr_(H, "conv3x3_wgrad", lambda g, x, cout, pad: (calls.update(K12=1), real_wgrad(g, x, cout, pad))[1])
    if path == "hand_written_convolutions":
        setattr_(H, "CONV3X3_MIN_PIXELS", 1)
        setattr_(H, "K12_MIN_PIXELS", 1)
        setenv("AURPPO_K12_ALL", "1")          # conv3x3_wgrad_ok otherwise leaves the 16 -> 32 block's weight gradient to the library
    if path == "k9_with_the_plane":
        encs = [m for m in pol.modules() if isinstance(m, base_encoder)]
        for m in encs:
            setattr_(m, "fused_first", False)
    return calls


def assert_path_ran(path, counts, calls, sd, n_backward):
    """The kernels a path names ran (``counts``: capture_routing's, ``calls``: select_path's) after one evaluate and ``n_backward``
    backward passes -- exact counts, so that a dispatch change that hands a block back to the library fails.  Per encoder: K10 or K9 with
    the plane for the first block, K9 for every other pooled block; on the hand-written path K11 for EVERY hidden convolution (6 at
    128 x 128, 5 at 84 x 84) and K12 for each of them in every backward pass."""
    pooled = sum(1 for _, _, kind in encoder_layers(sd, "actor") if kind == "pool")
    hidden = len(encoder_layers(sd, "actor")) - 1
    if path == "k9_with_the_plane":
        assert (counts["K10"], counts["K9_plane"], counts["K9"]) == (0, 2, 2 * pooled), counts
    else:
        assert (counts["K10"], counts["K9_plane"], counts["K9"]) == (2, 0, 2 * (pooled - 1)), counts
    if path == "hand_written_convolutions":
        assert (calls["K11"], calls["K12"]) == (2 * hidden, 2 * hidden * n_backward), calls


def path_evaluate(pol, case):
    """One ``policy.evaluate`` on the GPU with grad enabled; returns (log-prob, entropy, value, routing, counts)."""
    with capture_routing(pol) as (rec, counts):
        _, _, lp, ent, v = pol.evaluate(case["state"].cuda(), case["obs"].cuda(), case["act"].cuda())
    return lp, ent, v, list(rec), counts


def path_step(pol, case, lp, ent, v, vmode, packed, hyper=HYPER, norm_adv=True):
    """The PPO loss as ``robot_ppo.update`` forms it (``ops.ppo_loss`` / ``ppo_loss_packed``) and its backward pass through the path;
    returns the ``step``-shaped result (grads by name, logp, value, scalars)."""
    from aur_ppo_amd import hip_ops as H
    rec = case["rec"].cuda().contiguous()
    sc = torch.zeros(H.N_SCALARS, device="cuda")
    hv = {O.VLOSS_CLIPPED: H.VLOSS_CLIPPED, O.VLOSS_RETURNS: H.VLOSS_RETURNS}[vmode]
    if packed:
        loss = H.ppo_loss_packed(lp, v, ent, rec, hyper["clip"], hyper["ent_coef"], hyper["vf_coef"], norm_adv, hv, sc)
    else:
        ol, adv, ret, ov = (rec[:, k].contiguous() for k in range(4))
        loss = H.ppo_loss(lp, v, ent, ol, adv, ov, ret, hyper["clip"], hyper["ent_coef"], hyper["vf_coef"], norm_adv, hv, sc)
    for p in pol.parameters():
        p.grad = None
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in pol.named_parameters()}
    return dict(grads=grads, logp=lp.detach(), value=v.detach().reshape(-1), scalars=sc.clone())


_YS = {}


def gpu_yardstick(key, net, case, ref, vmode, hyper=HYPER):
    k = (key, routing_key(ref["routing"]), vmode)
    if k not in _YS:
        _YS[k] = yardstick(net, case, ref, vmode, "cuda", hyper=hyper)
    return _YS[k]
