"""Cases of the layered rollout step (hip_ops.mlp_layered_act: k_linear from prepared operand copies + K14 k_head_act) shared by the
GPU test (tests/test_layered_act_fp64_gpu.py), the host test that shows the bars can be met at these shapes
(tests/test_layered_act_host.py) and tools/layered_act_fp64_table.py.  A plain helper module: ``tests/ref64.py`` supplies the reference
(``act_reference``), the metric, ``safe_uniform`` and the bar (``MARGIN``), unchanged.

What the list covers: hidden 32 (TPR 8) to 1024 (TPR 256, four waves per row); one to three layers; D in {16, 64, 144, 256}; Gaussian
heads of 1, 6, 12, 16 actions and Categorical heads of 2, 5, 16; N of 1, 2, one row group plus a row (33 at hidden 1024), 256 = one
k_linear workgroup, 513 = two workgroups plus a row; the three observation regimes.  Seeds as test_act_kernel_matches_fp64:
``_mk("layered", ...).seed + 1``."""
import numpy as np
import torch

from tests import ref64 as R

# (hidden, layers, D, A, continuous, N, regime)
_SHAPES = [
    (256, 2, 64, 6, True, 257, "normal"),
    (160, 3, 144, 12, True, 65, "scaled"),
    (64, 1, 144, 1, True, 1, "normal"),
    (512, 2, 256, 16, False, 257, "bf16half"),
    (1024, 1, 64, 6, True, 33, "scaled"),
    (1024, 3, 256, 2, False, 300, "normal"),
    (160, 1, 16, 2, False, 2, "normal"),
    (256, 3, 256, 16, True, 513, "bf16half"),
    (512, 1, 16, 16, False, 31, "scaled"),
    (32, 2, 144, 6, True, 256, "normal"),
    (1024, 2, 144, 12, True, 1, "bf16half"),
    (32, 1, 144, 5, False, 77, "normal"),
]
CASES = [R._mk("layered", h, l, D, A, cont, N, False, 0, regime) for h, l, D, A, cont, N, regime in _SHAPES]
IDS = [R.case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def build(c):
    """Weights, observations, noise (uniform draws made margin-safe; ``moved`` counts them), the fp64 net and its rollout step."""
    rs = np.random.RandomState(c.seed + 1)
    sd = R.make_policy_sd(c.hidden, c.layers, c.D, c.A, c.cont, rs, 1e-3 if c.regime == "scaled" else 1.0)
    N = c.M
    obs = R.make_obs(N, c.D, c.regime, rs)
    net64 = R.make_net(sd)
    moved = 0
    if c.cont:
        noise = torch.from_numpy(rs.standard_normal((N, c.A)).astype(np.float32))
    else:
        noise = torch.from_numpy(rs.random_sample(N).astype(np.float32))
        moved = R.safe_uniform(net64, obs, noise)
    return dict(sd=sd, obs=obs, noise=noise, net64=net64, moved=moved, ref=R.act_reference(net64, obs, noise))


def torch_fp32_step(c, data, device, net=None):
    """The same formulas in plain fp32 torch on ``device`` (``net``: another fp32 formulation of the policy): value, action, log-prob.
    The Categorical head's log-prob is taken at the reference's index."""
    ref = data["ref"]
    net32 = R.make_net(data["sd"], torch.float32, device) if net is None else net
    with torch.no_grad():
        o, z = data["obs"].to(device), data["noise"].to(device)
        v = net32.critic(o)
        if c.cont:
            a = net32.actor(o) + net32.actor_logstd.exp() * z
            _, lp, _, _ = net32.evaluate(o, a)
        else:
            a = None
            _, lp, _, _ = net32.evaluate(o, ref["action"].to(device))
    return v.reshape(-1), a, lp


def metrics(c, ref, v, a, lp):
    """test_act_kernel_matches_fp64's metric: the worst error over the sum of the absolute terms behind each number."""
    out = {"value": float(((v.double().cpu().reshape(-1) - ref["value"].reshape(-1)).abs() / ref["fwd_scales"]["value"].reshape(-1)).max()),
           "logp": float(((lp.double().cpu() - ref["logp"]).abs() / ref["fwd_scales"]["logp"]).max())}
    if c.cont:
        out["action"] = float(((a.double().cpu() - ref["action"]).abs() / ref["fwd_scales"]["action"]).max())
    return out


def yardstick(c, data, device):
    """(Y, per-quantity metrics of fp32 torch on ``device``): Y floored at one fp32 ulp."""
    y = metrics(c, data["ref"], *torch_fp32_step(c, data, device))
    return max(max(y.values()), R.ULP32), y
