"""GPU: every MLP family -- K7 (k_mlp_step3, k_mlp_step2), K7w ids 1 / 3 / 2, the layered step and its native twin (k_linear + K13), and the
rollout steps K8, K8w and K14 behind k_linear -- at tanh's and the heads' extremes, against the fp64 reference of tests/ref64.py.

The regimes (tests/ref64_extremes.py: tanh saturated, e^{2x} overflowing, tanh in its linear range, sigma = e^-3 / e^2, a softmax whose
probabilities are exactly 0 in fp32) are where the kernels' own formulas differ from torch's, and where ``1 - 2 / (e^{2x} + 1)`` is
absolute-accurate, not relative-accurate: Y alone (plain fp32 torch) is no bar a correct kernel could meet there.  The bar is a BAND,
B = max(Y, F, P) with F and P two CPU renditions of the kernels' formulas (P: the +-1 ulp envelope of v_exp_f32 / v_rcp_f32), and the
margins are ref64's own: ``MARGIN`` for every gradient tensor and for the rollout step, ``MARGIN_SCALARS`` for the nine scalars; the rollout
step in ``deep`` has a class margin of its own (``ref64_extremes.MARGIN_ACT_DEEP``, from a CPU rendition of another summation order).
Every output must be finite; nothing is excluded.  tests/test_mlp_extremes_host.py shows on the CPU that a second rendition meets these
bars and which wrong computations they reject; DESIGN 2.6 has the figures.  M = 1000 throughout (tile and row edges are the business of
tests/test_mlp_fp64_gpu.py's cases), default tile order only.  Each test prints the kernel it ran and its ratios (``-s``)."""
import numpy as np
import pytest
import torch

from tests import ref64 as R
from tests import ref64_extremes as X

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(c):
    """Inputs, fp64 reference and the band of a case, computed once and shared by the builds of its family."""
    if c not in _CACHE:
        data = X.build_case(c)
        data["ref"] = R.reference_step(c, data)
        data["band"] = X.band_step(c, data, "cuda")
        data["gpu"] = R.gpu_inputs(c, data)
        del data["net64"]
        _CACHE[c] = data
    return _CACHE[c]


def _band_text(band):
    return ", ".join(f"{k} {v:.3e}" for k, v in band["parts"].items())


_FUSED = [(c, k) for c in X.K7_STEP + X.K7W1_STEP + X.K7W_WIDER_STEP for k in R.kernels_for(c)]


@pytest.mark.parametrize("c,k", _FUSED, ids=[f"{k.name}-{R.case_id(c)}" for c, k in _FUSED])
def test_fused_step_at_the_extremes(c, k, monkeypatch):
    data = _case(c)
    label = R.select_kernel(c, k, 0, monkeypatch.setenv)
    sc, g = R.kernel_step(c, data, R.gpu_policy(c, data["sd"]))
    torch.cuda.synchronize()
    print(f"\nband: {_band_text(data['band'])}")
    X.check_step_band(c, sc, g, data["ref"], data["band"], label)


@pytest.mark.parametrize("route", ["mlp_layered_step", "mlp_layered_step_native"])
@pytest.mark.parametrize("c", X.LAYERED_STEP, ids=R.case_id)
def test_layered_step_at_the_extremes(c, route):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    data = _case(c)
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    pol.load_state_dict(data["sd"])
    pol = pol.cuda()
    bucket = FlatBucket(pol.parameters())
    assert H.mlp_layout(pol, bucket) is None
    lay = H.mlp_layered_layout(pol, bucket)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (c.D, c.A, c.hidden, c.layers)
    assert [n for n, _ in pol.named_parameters()] == R.param_names(R.make_net(data["sd"])), "FlatBucket order"
    obs, act, rec, idx = data["gpu"]
    n = lay["n_params"]
    g = torch.full((bucket.flat_grad.numel() + 64,), float("nan"), device="cuda")
    sc = getattr(H, route)(obs, act, rec, idx, bucket.flat_param, lay, g, R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    torch.cuda.synchronize()
    assert bool(torch.isnan(g[n:]).all()), "the step wrote past n_params"
    print(f"\nband: {_band_text(data['band'])}")
    X.check_step_band(c, sc, g[:n], data["ref"], data["band"], f"layered: {route}")


# ---------------------------------------------------------------------------------- the rollout step
def _act_policy(c, sd):
    """(H, bucket, layout, the entry that runs this shape's rollout step, its label)."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    pol.load_state_dict(sd)
    pol = pol.cuda()
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layout(pol, bucket)
    if c.kind == "layered":
        assert lay is None
        lay = H.mlp_layered_layout(pol, bucket)
        assert lay is not None
        return H, bucket, lay, H.mlp_layered_act, "K14 behind k_linear (mlp_layered_act)"
    assert lay is not None and lay["wide"] == (c.kind == "k7w")
    return H, bucket, lay, H.mlp_act, "K8w" if lay["wide"] else "K8"


@pytest.mark.parametrize("c", X.ACT_CASES, ids=[{"k7": "K8-", "k7w": "K8w-", "layered": "K14-"}[c.kind] + R.case_id(c) for c in X.ACT_CASES])
def test_rollout_step_at_the_extremes(c):
    """Value, action and log-prob per sample within MARGIN x the band (``deep``: MARGIN_ACT_DEEP, the class margin ref64_extremes derives
    from two summation orders on the CPU); the Categorical index EQUAL for every sample (``peaked`` included: the draws keep BRANCH_EPS
    away from every edge of the fp64 CDF); the value-only call gives the same bits."""
    data = X.build_act(c)
    ref = data["ref"]
    band = X.band_act(c, data, "cuda")
    H, bucket, lay, act_fn, label = _act_policy(c, data["sd"])
    obs, noise = data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous()
    a, lp, v = act_fn(obs, noise, bucket.flat_param, lay)
    torch.cuda.synchronize()
    if not c.cont:
        assert torch.equal(a.long().cpu(), ref["action"]), int((a.long().cpu() != ref["action"]).sum())
    m = X.act_metrics(c, ref, v, a, lp)
    B = band["B"]
    print(f"\n[{label}] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / B:.2f} x B" for n, x in m.items()) + f" (band: {_band_text(band)}; moved {data['moved']})")
    for n, x in m.items():
        assert x <= X.act_margin(c) * B, (label, n, x, B, x / B, X.act_margin(c))
    _, _, v2 = act_fn(obs, None, bucket.flat_param, lay)
    assert torch.equal(v2, v)


# ---------------------------------------------------------------------------------- the tanh itself
NONFINITE = (float("inf"), float("-inf"), float("nan"))


def _check_nonfinite(y, label):
    """tanh(+inf) = 1, tanh(-inf) = -1, exactly; NaN -> NaN."""
    y = [float(t) for t in y]
    print(f"[{label}] tanh(+inf, -inf, nan) = {y}")
    assert y[0] == 1.0 and y[1] == -1.0 and np.isnan(y[2]), (label, y)


def test_tanh_of_k_linear_epilogue():
    """``linear_bias_act(x, I16, 0, act=1)`` is k_linear's tanh of x itself: with ``act=0`` the same call returns x bit for bit (the three
    bf16 planes of x times 1.0 sum exactly).  The non-finite arguments arrive through the bias (0 * inf in the product would be NaN)."""
    from aur_ppo_amd import hip_ops as H
    x = X.tanh_sweep_points(width=16).view(-1, 16).cuda()
    eye, zero = torch.eye(16, device="cuda"), torch.zeros(16, device="cuda")
    y0 = H.linear_bias_act(x, eye, zero, act=0)
    torch.cuda.synchronize()
    nz = x != 0                                 # (-0 comes back as +0: the accumulator starts at +0)
    assert torch.equal(y0.view(torch.int32)[nz], x.view(torch.int32)[nz]) and bool((y0[~nz] == 0).all()), "x . I is not x"
    y = H.linear_bias_act(x, eye, zero, act=1)
    torch.cuda.synchronize()
    X.check_tanh_sweep(x, y, "k_linear epilogue: linear_bias_act act=1")
    bias = torch.zeros(16, device="cuda")
    bias[:3] = torch.tensor(NONFINITE, device="cuda")
    y = H.linear_bias_act(torch.zeros(1, 16, device="cuda"), eye, bias, act=1)
    torch.cuda.synchronize()
    _check_nonfinite(y[0, :3].cpu(), "k_linear epilogue")
    assert bool((y[0, 3:] == 0).all())


def test_tanh_fast_through_k8w():
    """K8w with a 1 x 64, D 64 policy whose critic is W0 = I, b0 = 0 and a one-hot head row j: value = tanh_fast(x_j) exactly (fp32 matrix
    products of one non-zero term).  Column j of the sweep per launch; the non-finite arguments through b0[j], one at a time."""
    from aur_ppo_amd import hip_ops as H
    c = X.mk("k7w", 64, 1, 64, 6, True, "saturated", False, 0)
    sd = R.make_policy_sd(64, 1, 64, 6, True, np.random.RandomState(c.seed))
    sd["critic.net.0.weight"] = torch.eye(64)
    sd["critic.net.0.bias"] = torch.zeros(64)
    sd["critic.net.2.bias"] = torch.zeros(1)
    _pol, bucket, lay = R.gpu_policy(c, sd)
    assert lay["wide"]
    off = lay["offsets"]                       # {w_l, b_l} for l = 0 .. L of the actor, then of the critic, then actor_logstd
    assert len(off) == 9
    b0, head = off[5], off[6]
    assert torch.equal(bucket.flat_param[off[4]:off[4] + 64 * 64].view(64, 64), torch.eye(64, device="cuda"))
    x = X.tanh_sweep_points(width=64).view(-1, 64).cuda().contiguous()
    y = torch.empty_like(x)
    for j in range(64):
        bucket.flat_param[head:head + 64] = 0.0
        bucket.flat_param[head + j] = 1.0
        _, _, v = H.mlp_act(x, None, bucket.flat_param, lay)
        y[:, j] = v
    torch.cuda.synchronize()
    X.check_tanh_sweep(x, y, "K8w: tanh_fast")
    got = []
    zeros = torch.zeros(1, 64, device="cuda")
    for val in NONFINITE:
        bucket.flat_param[b0 + 63] = val
        _, _, v = H.mlp_act(zeros, None, bucket.flat_param, lay)
        got.append(float(v[0]))
    _check_nonfinite(got, "K8w")
