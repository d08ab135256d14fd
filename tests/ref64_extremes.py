"""The MLP kernels at tanh's and the heads' extremes: regimes of the policy, fp32 renditions of the kernels' formulas, and the band of
correct fp32 computations the kernels are judged against.  A plain helper module on top of ``tests/ref64.py`` (reference, metric,
margins and ``make_records_safe`` / ``safe_uniform`` unchanged); DESIGN 2.6 has the figures.

Regimes: a transform of the state dict ``ref64.make_policy_sd`` returns (the same generator draws as the normal cases, then scaled),
on ``make_obs(..., "normal")`` observations.  ``build_case`` / ``build_act`` assert each regime's CONDITION in fp64 on the rows the
kernel will see, per net and per hidden layer:

  saturated   every hidden layer x 4          share |t| > 0.999 >= 0.25, share |t| < 0.9 >= 0.25, max |x| < 44
  deep        every hidden layer x 64         share |x| > 44.5 >= 0.40 (e^{2x} overflows or is 0), share |t| < 0.9 >= 0.01
  linear      first layer x 1e-3              layer 0: max |x| < 0.01
  linear_all  every hidden layer x 1e-2       every hidden layer: max |x| < 0.1
  tight/loose actor_logstd = -3 / +2          (Gaussian) actions drawn from the fp64 policy, mu64 + sigma * eps: z / sigma stays O(1)
  peaked      actor head x 40                 (Categorical) rows with max p > 1 - 1e-6 >= 0.25, lowest log-prob < -80; actions stay
                                              uniform draws, so improbable actions are taken

Renditions: ``ref64.make_alternative_fp32_net`` (exact six-product matrix products, the kernels' log-prob and softmax forms) with its
tanh swapped for an autograd function whose backward is g * (1 - t * t) from the stored output, as the kernels form tanh':

  F    t = 1 - 2 / (exp(2x) + 1)
  F2   t = 1 - 2 * (1 / (exp2(x * 2.8853900817779268) + 1))
  P    F2 with the exponential and the reciprocal each multiplied by 1 +- 2^-23 (signs from RandomState(case seed)): the +-1 ulp
       envelope of the two instructions.  The perturbed reciprocal is kept <= 1 (the reciprocal of exactly 1.0 is exact), so that P,
       like the kernels, never leaves [-1, 1]: the band it spans asks no less for that.

Band: B = max(Y, F, P), each the computation's worst-tensor metric as ``ref64.yardstick_step`` defines Y (plain fp32 torch on the
device; F and P on the CPU).  A bar is ``ref64.MARGIN * B`` (gradients) / ``ref64.MARGIN_SCALARS * max(Bs)`` (scalars)."""
from __future__ import annotations

import collections

import numpy as np
import torch
from torch import nn

from tests import ref64 as R

GAUSS_REGIMES = ("saturated", "deep", "linear", "linear_all", "tight", "loose")
CAT_REGIMES = ("saturated", "deep", "linear", "peaked")
REGIMES = GAUSS_REGIMES + ("peaked",)
M_STEP = 1000          # at M 65 the band is a draw; tile and row edges are the business of ref64's own cases
N_ACT = 257
K_TANH = float(np.float32(2.8853900817779268))      # csrc/mlp_common.h: kTanhC
EPS23 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ regimes
def apply_regime(sd, regime):
    """A copy of the state dict ``sd`` transformed into ``regime`` (fp32 products of fp32 weights: what the kernels will read)."""
    _D, _A, _hidden, layers, cont = R.net_shape(sd)
    out = collections.OrderedDict((k, v.clone()) for k, v in sd.items())

    def scale(net, l, f):
        for kind in ("weight", "bias"):
            out[f"{net}.net.{2 * l}.{kind}"] *= f
    if regime in ("saturated", "deep", "linear_all"):
        f = {"saturated": 4.0, "deep": 64.0, "linear_all": 1e-2}[regime]
        for net in ("actor", "critic"):
            for l in range(layers):
                scale(net, l, f)
    elif regime == "linear":
        scale("actor", 0, 1e-3), scale("critic", 0, 1e-3)
    elif regime in ("tight", "loose"):
        assert cont, regime
        out["actor_logstd"].fill_(-3.0 if regime == "tight" else 2.0)
    elif regime == "peaked":
        assert not cont, regime
        scale("actor", layers, 40.0)
    else:
        raise ValueError(regime)
    return out


def hidden_preactivations(net64, obs):
    """{(net, layer): fp64 pre-activations (rows, hidden)} of every hidden layer of both nets on ``obs``."""
    got, hooks = {}, []
    for which in ("actor", "critic"):
        seq = getattr(net64, which).net
        for l in range((len(seq) - 1) // 2):
            hooks.append(seq[2 * l].register_forward_hook((lambda key: lambda _m, _i, o: got.__setitem__(key, o.detach()))((which, l))))
    with torch.no_grad():
        net64.actor(obs.double()), net64.critic(obs.double())
    for h in hooks:
        h.remove()
    return got


def check_condition(regime, net64, obs):
    """Assert the regime's condition on the rows ``obs`` and return what was measured: {name: (lowest, highest) over nets and layers}."""
    pre = hidden_preactivations(net64, obs)
    found = collections.OrderedDict()

    def note(name, v):
        lo, hi = found.get(name, (v, v))
        found[name] = (min(lo, v), max(hi, v))
    for (which, l), x in pre.items():
        t, ax = torch.tanh(x).abs(), x.abs()
        share = lambda m: float(m.double().mean())
        if regime == "saturated":
            a, b, mx = share(t > 0.999), share(t < 0.9), float(ax.max())
            note("share |t| > 0.999", a), note("share |t| < 0.9", b), note("max |x|", mx)
            assert a >= 0.25 and b >= 0.25 and mx < 44, (regime, which, l, a, b, mx)
        elif regime == "deep":
            a, b = share(ax > 44.5), share(t < 0.9)
            note("share |x| > 44.5", a), note("share |t| < 0.9", b)
            assert a >= 0.40 and b >= 0.01, (regime, which, l, a, b)
        elif regime == "linear" and l == 0:
            note("layer 0 max |x|", float(ax.max()))
            assert float(ax.max()) < 0.01, (regime, which, l, float(ax.max()))
        elif regime == "linear_all":
            note("max |x|", float(ax.max()))
            assert float(ax.max()) < 0.1, (regime, which, l, float(ax.max()))
    if regime == "peaked":
        with torch.no_grad():
            lp = torch.log_softmax(net64.actor(obs.double()), 1)
        a, lo = float((lp.max(1).values.exp() > 1 - 1e-6).double().mean()), float(lp.min())
        note("rows with max p > 1 - 1e-6", a), note("lowest log-prob", lo)
        assert a >= 0.25 and lo < -80, (regime, a, lo)
    return found


# ------------------------------------------------------------------------------------------------ cases
def mk(kind, hidden, layers, D, A, cont, regime, norm_adv, vmode, packed=False, M=M_STEP):
    return R._mk(kind, hidden, layers, D, A, cont, M, norm_adv, vmode, regime, "perm", packed)


def _spread(kind, hidden, layers, D, A, cont, shift):
    """One case per regime of the head, value modes 0 / 1 / 2, both normalisations and packed records dealt over the list."""
    regimes = GAUSS_REGIMES if cont else CAT_REGIMES
    return [mk(kind, hidden, layers, D, A, cont, r, (i + shift) % 2 == 0, (i + shift) % 3, (i + shift) % 4 >= 2) for i, r in enumerate(regimes)]


# (family / shape: ref64.kernels_for gives K7's and K7w's builds; the layered shapes run mlp_layered_step and its native twin)
K7_STEP = _spread("k7", 64, 2, 16, 6, True, 0) + _spread("k7", 64, 2, 4, 6, False, 1)
K7W1_STEP = _spread("k7w", 64, 3, 15, 6, True, 2) + _spread("k7w", 32, 1, 5, 2, False, 3)
K7W_WIDER_STEP = _spread("k7w", 96, 2, 65, 6, True, 1) + _spread("k7w", 128, 1, 4, 16, False, 2)
LAYERED_STEP = _spread("layered", 160, 2, 64, 6, True, 3) + _spread("layered", 160, 1, 16, 16, False, 0)
# a case whose own seed misses its regime's condition gets another seed, never another condition: 1 x 128, D 4, A 16 peaked has 0.244
# of its rows at max p > 1 - 1e-6 with the seed ``ref64._mk`` gives it (0.25 asked), 0.383 with this one
_SEEDS = {"k7w-1x128-D4-A16-cat-M1000-raw-v2-peaked-perm": 2563}
K7W_WIDER_STEP = [c._replace(seed=_SEEDS.get(R.case_id(c), c.seed)) for c in K7W_WIDER_STEP]
STEP_CASES = K7_STEP + K7W1_STEP + K7W_WIDER_STEP + LAYERED_STEP
assert len({R.case_id(c) for c in STEP_CASES}) == len(STEP_CASES) and sum(R.case_id(c) in _SEEDS for c in STEP_CASES) == len(_SEEDS)


def _act_cases(kind, hidden, layers, D):
    return ([mk(kind, hidden, layers, D, 6, True, r, False, 0, M=N_ACT) for r in GAUSS_REGIMES]
            + [mk(kind, hidden, layers, D, 6, False, r, False, 0, M=N_ACT) for r in CAT_REGIMES])


# K8 (2 x 64), K8w (1 x 64 over D 64; 3 x 128 over D 128), K14 behind k_linear (2 x 160 over D 64)
ACT_CASES = _act_cases("k7", 64, 2, 16) + _act_cases("k7w", 64, 1, 64) + _act_cases("k7w", 128, 3, 128) + _act_cases("layered", 160, 2, 64)


def build_case(c):
    """``ref64.build_case`` for a regime of this module: the same draws in the same order, the state dict transformed, the actions of
    ``tight`` / ``loose`` drawn from the fp64 policy.  Asserts the regime's condition on the minibatch's rows (``cond``: what it found)
    and, through ``make_records_safe``, that no sample is within BRANCH_EPS of a decision."""
    rs = np.random.RandomState(c.seed)
    sd = apply_regime(R.make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs), c.regime)
    assert c.index == "perm"
    B = c.M + 37
    idx = torch.from_numpy(rs.permutation(B)[:c.M].astype(np.int32))
    obs = R.make_obs(B, c.D, "normal", rs)
    net64 = R.make_net(sd)
    if c.cont:
        eps = torch.from_numpy(rs.standard_normal((B, c.A)).astype(np.float32))
        act = eps
        if c.regime in ("tight", "loose"):
            with torch.no_grad():
                act = (net64.actor(obs.double()) + net64.actor_logstd.exp() * eps.double()).float()
    else:
        act = torch.from_numpy(rs.randint(0, c.A, size=B).astype(np.float32))
    with torch.no_grad():
        _, lp, _, v = net64.evaluate(obs.double(), act.double() if c.cont else act.long())
    v = v.reshape(-1)
    rec = torch.stack([lp + 0.2 * torch.from_numpy(rs.standard_normal(B)), 2 * torch.from_numpy(rs.standard_normal(B)),
                       v + torch.from_numpy(rs.standard_normal(B)), v + 0.25 * torch.from_numpy(rs.standard_normal(B))], 1).float()
    li = idx.long()
    moved = R.make_records_safe(lp[li], v[li], rec, idx, R.HYPER["clip"], c.norm_adv, c.vmode)
    cond = check_condition(c.regime, net64, obs[li])
    return dict(sd=sd, net64=net64, obs=obs, act=act, rec=rec.contiguous(), idx=idx, moved=moved, cond=cond)


def build_act(c):
    """The rollout step's inputs in a regime (``layered_act_cases.build``'s draws): weights, observations, noise (uniform draws made
    margin-safe), the fp64 net and its rollout step.  The Gaussian action is mu + sigma * noise by construction."""
    rs = np.random.RandomState(c.seed + 1)
    sd = apply_regime(R.make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs), c.regime)
    N = c.M
    obs = R.make_obs(N, c.D, "normal", rs)
    net64 = R.make_net(sd)
    moved = 0
    if c.cont:
        noise = torch.from_numpy(rs.standard_normal((N, c.A)).astype(np.float32))
    else:
        noise = torch.from_numpy(rs.random_sample(N).astype(np.float32))
        moved = R.safe_uniform(net64, obs, noise)
    cond = check_condition(c.regime, net64, obs)
    return dict(sd=sd, obs=obs, noise=noise, net64=net64, moved=moved, cond=cond, ref=R.act_reference(net64, obs, noise))


# ------------------------------------------------------------------------------------------------ renditions
def _round_bits(e, bits):
    """``e`` rounded to ``bits`` significant bits (inf and 0 stay)."""
    m, ex = torch.frexp(e)
    k = float(2 ** bits)
    return torch.where(torch.isfinite(e), torch.ldexp(torch.round(m * k) / k, ex), e)


class _TanhFn(torch.autograd.Function):
    """kind: F / F2 / P (the renditions); exp12 (F2 with e^{2x} good to 2^-12 only) and over1 (F2 + 2^-22: |t| above 1), two mutants."""

    @staticmethod
    def forward(ctx, x, kind, rs):
        if kind == "F":
            t = 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)
        else:
            e = torch.exp2(x * K_TANH)
            if kind == "P":
                e = e * torch.from_numpy((1.0 + EPS23 * (2 * rs.randint(0, 2, size=tuple(x.shape)) - 1)).astype(np.float32))
            elif kind == "exp12":
                e = _round_bits(e, 12)
            r = 1.0 / (e + 1.0)
            if kind == "P":
                r = torch.clamp(r * torch.from_numpy((1.0 + EPS23 * (2 * rs.randint(0, 2, size=tuple(x.shape)) - 1)).astype(np.float32)), max=1.0)
            t = 1.0 - 2.0 * r
            if kind == "over1":
                t = t + 2.0 ** -22
        ctx.save_for_backward(t)
        return t

    @staticmethod
    def backward(ctx, g):
        t, = ctx.saved_tensors
        return g * (1.0 - t * t), None, None


class _Tanh(nn.Module):
    def __init__(self, kind, rs):
        super().__init__()
        self.kind, self.rs = kind, rs

    def forward(self, x):
        return _TanhFn.apply(x, self.kind, self.rs)


TANH_KINDS = ("F", "F2", "P", "exp12", "over1", "autograd")
HEAD_KINDS = ("kernel", "no_max", "log_p")


def make_rendition_net(sd, kind, seed=0, head="kernel"):
    """``ref64.make_alternative_fp32_net`` with the tanh of ``kind`` (``autograd``: ``ref64._FastTanh`` as it is, tanh' from autograd of
    the formula -- a mutant).  ``head``: ``kernel`` (the kernels' forms), or a mutant of the Categorical head: ``no_max`` (softmax
    without the max subtracted), ``log_p`` (entropy as -sum p log p with the logarithm taken of the fp32 probability)."""
    assert kind in TANH_KINDS and head in HEAD_KINDS
    net = R.make_alternative_fp32_net(sd)
    rs = np.random.RandomState(seed)
    if kind != "autograd":
        for which in ("actor", "critic"):
            seq = getattr(net, which).net
            for i in range(len(seq)):
                if isinstance(seq[i], R._FastTanh):
                    seq[i] = _Tanh(kind, rs)
    if head != "kernel":
        assert not net.continuous

        def evaluate(obs, act):
            mu, v = net.actor(obs), net.critic(obs)
            mx = mu.max(1, keepdim=True).values if head == "log_p" else torch.zeros_like(mu[:, :1])
            ex = torch.exp(mu - mx)
            s = ex.sum(1, keepdim=True)
            lp = mu - (mx + torch.log(s))
            ent = -((ex / s) * torch.log(ex / s)).sum(1) if head == "log_p" else -(torch.exp(lp) * lp).sum(1)
            return act, lp.gather(1, act[:, None])[:, 0], ent, v
        net.evaluate = evaluate
    return net


class _RunningLinear(nn.Module):
    """x @ W^T + b with each output a RUNNING fp32 sum over k (exact products, one rounding per term, as a chain of fused
    multiply-adds or of fp32 matrix instructions leaves it) in a chosen order: ``rev`` (k from the last to the first) or ``four`` (four
    interleaved partial sums, added pairwise at the end).  Forward only: the rollout step."""

    def __init__(self, lin, order):
        super().__init__()
        assert order in ("rev", "four")
        self.weight, self.bias, self.order = lin.weight, lin.bias, order

    def _chain(self, x, ks):
        acc = torch.zeros(x.shape[0], self.weight.shape[0])
        for k in ks:
            acc = (acc.double() + x[:, k, None].double() * self.weight[None, :, k].double()).float()
        return acc

    def forward(self, x):
        K = x.shape[1]
        if self.order == "rev":
            return self._chain(x, reversed(range(K))) + self.bias
        p = [self._chain(x, range(j, K, 4)) for j in range(4)]
        return ((p[0] + p[1]) + (p[2] + p[3])) + self.bias


def make_order_net(sd, order, kind="F2"):
    """The rendition ``kind`` with its matrix products as running fp32 sums in ``order`` instead of exact ones: what ANOTHER summation
    order of the same fp32 product gives (plain fp32 torch on the CPU runs k upwards).  The rollout step's class margin in ``deep``
    comes from it (``MARGIN_ACT_DEEP``)."""
    net = make_rendition_net(sd, kind)
    with torch.no_grad():
        for which in ("actor", "critic"):
            seq = getattr(net, which).net
            for i in range(len(seq)):
                if isinstance(seq[i], R.EmulatedLinear):
                    seq[i] = _RunningLinear(seq[i], order)
    return net


def rendition_step(c, data, kind, head="kernel", net=None):
    """One fp32 step of a rendition (or of ``net``) on the CPU, as ``ref64.run_step`` returns it."""
    li = data["idx"].long()
    net = make_rendition_net(data["sd"], kind, c.seed, head) if net is None else net
    return R.run_step(net, data["obs"][li], data["act"][li], data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"],
                      c.norm_adv, c.vmode)


# ------------------------------------------------------------------------------------------------ the band
def band_step(c, data, device, kinds=("F", "P")):
    """dict(B, Bs, parts, tensors): B = max(Y, renditions ``kinds``), each the computation's worst-tensor metric against
    ``data["ref"]``; Bs per scalar likewise, with ``yardstick_step``'s one-ulp floor; ``parts`` = {"Y" / kind: worst-tensor metric}.
    Y runs on ``device``, the renditions on the CPU."""
    ref = data["ref"]
    Y, Ys, _ = R.yardstick_step(c, data, device)
    parts, Bs = collections.OrderedDict(Y=Y), dict(Ys)
    for kind in kinds:
        got = rendition_step(c, data, kind)
        parts[kind] = max(R.grad_metrics(got["flat"], ref).values())
        for n, m in R.scalar_metrics(got["scalars"], ref).items():
            Bs[n] = max(Bs[n], m)
    return dict(B=max(parts.values()), Bs=Bs, parts=parts)


def check_step_band(c, sc, g, ref, band, label=""):
    """``ref64.check_step`` with the band in Y's place: every gradient tensor <= MARGIN * B, every scalar <= MARGIN_SCALARS * max(Bs),
    every output finite (``grad_metrics`` / ``scalar_metrics`` assert it), nothing excluded."""
    assert c.M >= R.TINY_M
    return R.check_step(c, sc, g, ref, band["B"], band["Bs"], label)


# The rollout step in ``deep``: a row's value / action error is the rounding of the pre-activations (partial sums of magnitude ~64, so
# ~1e-5 absolute) of the one or two units in 64 that are NOT saturated, carried by tanh' ~ 1 -- per row a draw of the product's summation
# order, and the metric is the worst of 257 rows.  Two fp32 summation orders of the same product (``make_order_net``) lie up to 2.66 x
# the band apart over 384 CPU draws (median 0.6 - 1.25; tests/test_mlp_extremes_host.py re-measures it), where the step at M 1000, whose
# gradients average over the rows, and every other regime stay under MARGIN.  As MARGIN_TINY_M and MARGIN_SCALARS, the class margin is
# that worst rounded up to the next power of two; it is not taken from a kernel.
MARGIN_ACT_DEEP = 4.0


def act_margin(c):
    return MARGIN_ACT_DEEP if c.regime == "deep" else R.MARGIN


def act_metrics(c, ref, v, a, lp):
    """``layered_act_cases.metrics``: value, log-prob (and the Gaussian action) over the terms behind each; all must be finite."""
    from tests import layered_act_cases as LA
    for n, x in (("value", v), ("logp", lp)) + ((("action", a),) if c.cont else ()):
        assert bool(torch.isfinite(x).all()), f"{n}: non-finite"
    return LA.metrics(c, ref, v, a, lp)


def band_act(c, data, device, kinds=("F", "P")):
    """dict(B, parts): the rollout step's band, max over fp32 torch on ``device`` and the renditions on the CPU of the worst of
    value / action / log-prob, floored at one fp32 ulp (``layered_act_cases.yardstick``)."""
    from tests import layered_act_cases as LA
    parts = collections.OrderedDict(Y=max(act_metrics(c, data["ref"], *LA.torch_fp32_step(c, data, device)).values()))
    for kind in kinds:
        net = make_rendition_net(data["sd"], kind, c.seed)
        parts[kind] = max(act_metrics(c, data["ref"], *LA.torch_fp32_step(c, data, "cpu", net=net)).values())
    return dict(B=max(max(parts.values()), R.ULP32), parts=parts)


# ------------------------------------------------------------------------------------------------ the tanh itself
TANH_BOUND = 2.0 ** -21      # exp 1 ulp x e/(e+1), the add 1/2 ulp, the reciprocal 1 ulp: <= 4 units of 2^-24 on r; 2r <= 2 and the last
                             # subtraction: <= 8 units.  (The +-1 ulp rendition reaches 7.5, F 3.0.)
SPECIALS = (9.0, 9.01, 10.0, 44.0, 44.4, 45.0, 88.0, 89.0, 1e4, 3e38)


def tanh_sweep_points(n_dense=1 << 20, width=16):
    """fp32 sweep of finite x, padded with zeros to a multiple of ``width``: >= 10^6 points of [-12, 12], +-logspace(1e-30 .. 1),
    +-SPECIALS and +-0."""
    dense = np.linspace(-12.0, 12.0, n_dense)
    logs = np.logspace(-30, 0, 3001)
    sp = np.array(SPECIALS)
    x = np.concatenate([dense, logs, -logs, sp, -sp, [0.0, -0.0]]).astype(np.float32)
    x = np.concatenate([x, np.zeros(-x.size % width, np.float32)])
    return torch.from_numpy(x)


def check_tanh_sweep(x, y, label):
    """The assertions on finite ``x``: |y - tanh64(x)| <= 2^-21, |y| <= 1, y = +-1 exactly at |x| >= 10.  Prints and returns the
    measured maximum in units of 2^-24."""
    x, y = x.detach().cpu().reshape(-1), y.detach().cpu().reshape(-1)
    assert x.numel() == y.numel() and bool(torch.isfinite(x).all())
    assert bool(torch.isfinite(y).all()), f"{label}: non-finite tanh of a finite x"
    err = (y.double() - torch.tanh(x.double())).abs()
    i = int(err.argmax())
    units = float(err[i]) / R.ULP32
    print(f"\n[{label}] {x.numel()} points: max |y - tanh64(x)| = {units:.2f} units of 2^-24 at x = {float(x[i])!r} (bound 8); max |y| = {float(y.abs().max())!r}")
    assert float(y.abs().max()) <= 1.0, (label, float(y.abs().max()))
    far = x.abs() >= 10.0
    assert torch.equal(y[far], torch.sign(x[far])), (label, "tanh is not exactly +-1 at |x| >= 10")
    assert float(err[i]) <= TANH_BOUND, (label, float(x[i]), float(y[i]), units)
    return units
