"""GPU: the layered rollout step on the small-M products, both nets' layer in one launch (``hip_ops.mlp_layered_act(paired=True)``:
k_linear_pair per layer + K14, L + 1 launches) against the unpaired route (k_linear per net and layer + K14).  The small tile keeps a
row's k-steps, their order and their arithmetic, so everything here is bit equality.

T5  paired equals unpaired in actions, log-prob and value; shapes of tests/layered_act_cases.py / tests/layered_ragged_cases.py's
    kinds -- 2 x 256 Gaussian, 1 x 1024 Categorical, 3 x 160 at a ragged state width (17: layer 0 on the tail builds), 2 x 32 -- at
    N of 1, 257 and 513 rows; and the value-only call.
T6  ``mlp_layered_step`` over rows of a paired rollout reports old_kl, kl and clipfrac of exactly 0: the rollout's log-prob and value
    are the update's (tests/test_layered_act_fp64_gpu.py has the unpaired route's).
T7  a paired step captured on one stream (the prepare launches inside it) and replayed on new observations equals the eager step.
T8  the trainer: T = 4 rollout steps and the bootstrap of a 2 x 256 policy on 64 synthetic envs with ``AURPPO_LAYERED_ACT=1``, with and
    without ``AURPPO_LAYERED_ACT_PAIRED=1``, each in a fresh process: the rollout buffers are bit-equal."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# (hidden, layers, D, A, continuous)
SHAPES = [(256, 2, 64, 6, True), (1024, 1, 64, 16, False), (160, 3, 17, 6, True), (32, 2, 144, 6, True)]
IDS = ["2x256-gauss", "1x1024-cat", "3x160-D17-gauss", "2x32-gauss"]


def _policy(hidden, layers, D, A, cont, seed):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(D, (A,) if cont else A, hidden, layers, 0.0, cont).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layered_layout(pol, bucket, any_state=True)
    assert lay is not None and H.mlp_layout(pol, bucket) is None
    return H, bucket, lay


def _inputs(N, D, A, cont, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn(N, D, device="cuda", generator=g)
    noise = torch.randn(N, A, device="cuda", generator=g) if cont else torch.rand(N, device="cuda", generator=g)
    return obs, noise


# ---------------------------------------------------------------------------------- T5
@pytest.mark.parametrize("N", [1, 257, 513])
@pytest.mark.parametrize("hidden,layers,D,A,cont", SHAPES, ids=IDS)
def test_paired_act_equals_unpaired_act(hidden, layers, D, A, cont, N):
    H, bucket, lay = _policy(hidden, layers, D, A, cont, hidden + N)
    obs, noise = _inputs(N, D, A, cont, 7 * N + hidden)
    a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay)
    a, lp, v = a.clone(), lp.clone(), v.clone()
    ap, lpp, vp = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, paired=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ap).all()) and bool(torch.isfinite(lpp).all()) and bool(torch.isfinite(vp).all())
    assert torch.equal(ap, a) and torch.equal(lpp, lp) and torch.equal(vp, v)
    wop = H.mlp_layered_prepare(bucket.flat_param, lay)                      # from copies prepared once, into the caller's rows
    outs = (torch.empty_like(a), torch.empty_like(lp), torch.empty_like(v))
    got = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, *outs, wop=wop, paired=True)
    assert all(x is y for x, y in zip(got, outs)) and torch.equal(got[0], a) and torch.equal(got[1], lp) and torch.equal(got[2], v)
    a0, lp0, v0 = H.mlp_layered_act(obs, None, bucket.flat_param, lay, paired=True)          # the bootstrap: the critic alone
    assert a0 is None and lp0 is None and torch.equal(v0, v)
    assert torch.equal(H.mlp_layered_act(obs, None, bucket.flat_param, lay)[2], v)


def test_paired_act_equals_unpaired_act_on_the_two_column_block_builds():
    """1 x 1024 at 2049 rows: the paired launch has 2 x 17 x 16 = 544 two-block workgroups, where it takes the NB = 2 builds
    (bf3_gemm.h::bf3_small_grid; every shape above stays on NB = 1); the bootstrap's single product stays on NB = 1."""
    hidden, layers, D, A, N = 1024, 1, 17, 16, 2049
    H, bucket, lay = _policy(hidden, layers, D, A, False, 5)
    obs, noise = _inputs(N, D, A, False, 6)
    a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay)
    ap, lpp, vp = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, paired=True)
    assert torch.equal(ap, a) and torch.equal(lpp, lp) and torch.equal(vp, v)
    assert torch.equal(H.mlp_layered_act(obs, None, bucket.flat_param, lay, paired=True)[2], v)


# ---------------------------------------------------------------------------------- T6
def test_update_step_over_a_paired_rollout_has_zero_kl():
    hidden, layers, D, A, N, M = 256, 2, 64, 6, 513, 300
    H, bucket, lay = _policy(hidden, layers, D, A, True, hidden + N)
    obs, noise = _inputs(N, D, A, True, N * 7 + M)
    g = torch.Generator(device="cuda").manual_seed(5)
    a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, paired=True)
    rec = torch.stack([lp, torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g), v], 1).contiguous()
    idx = torch.randperm(N, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    grad = torch.empty_like(bucket.flat_grad)
    sc = H.mlp_layered_step(obs, a, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED).cpu()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(grad[:lay["n_params"]]).all())
    print(f"\npaired rollout, {layers} x {hidden}: old_kl {float(sc[H.S_OLD_KL])!r}, kl {float(sc[H.S_KL])!r}, clipfrac {float(sc[H.S_CLIPFRAC])!r}")
    assert float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0


# ---------------------------------------------------------------------------------- T7
def test_captured_paired_step_replays_on_new_observations():
    hidden, layers, D, A, N = 256, 2, 64, 6, 257
    H, bucket, lay = _policy(hidden, layers, D, A, True, 11)
    obs, noise = _inputs(N, D, A, True, 12)
    outs = (torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda"))

    def step():
        H.mlp_layered_act(obs, noise, bucket.flat_param, lay, *outs, paired=True)      # prepares inside: 2 L + L + 1 launches, one stream

    step()                                      # eager once: the workspaces exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in range(2):
        new_obs, new_noise = _inputs(N, D, A, True, 100 + k)
        obs.copy_(new_obs)
        noise.copy_(new_noise)
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = H.mlp_layered_act(new_obs, new_noise, bucket.flat_param, lay)            # eager, unpaired, buffers of its own
        torch.cuda.synchronize()
        for g_, w_ in zip(got, want):
            assert bool(torch.isfinite(g_).all()) and torch.equal(g_, w_), k


# ---------------------------------------------------------------------------------- T8
def _child(out_path):
    """One rollout and its bootstrap as the trainer runs them, with whatever switches the environment sets; the buffers go to a file."""
    from tests.test_layered_act_ppo_gpu import _agent, _hp
    torch.manual_seed(3)
    a = _agent(_hp(num_steps=4))
    assert a._mlp_layered_act is not None and a._act_paired == (os.environ.get("AURPPO_LAYERED_ACT_PAIRED", "0") != "0")
    a.seed_all(1)
    obs = torch.as_tensor(a.envs.reset(seed=list(range(a.num_envs)))[0], dtype=torch.float32).to(a.device)
    for t in (a.buffer.values, a.buffer.log_probs, a.buffer.actions):
        t.fill_(float("nan"))
    done = torch.zeros(a.num_envs, device=a.device)
    next_obs, next_done, _ = a._rollout_steps(obs, done, 0, None)
    ret, adv = a.advantages(next_obs, next_done)
    torch.cuda.synchronize()
    b = a.buffer
    torch.save({k: t.detach().cpu() for k, t in dict(states=b.states, actions=b.actions, log_probs=b.log_probs, values=b.values,
                                                       rewards=b.rewards, ret=ret, adv=adv).items()}, out_path)


def test_trainer_rollout_buffers_are_bit_equal_with_the_switch(tmp_path):
    procs = []
    for paired in (False, True):
        env = {k: v for k, v in os.environ.items() if k not in ("AURPPO_LAYERED_ACT_PAIRED", "AURPPO_LAYERED_STEP")}
        env["AURPPO_LAYERED_ACT"] = "1"
        if paired:
            env["AURPPO_LAYERED_ACT_PAIRED"] = "1"
        out = str(tmp_path / f"rollout_{int(paired)}.pt")
        procs.append((out, subprocess.Popen([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT,
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    got = []
    for out, p in procs:
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, log[-2000:]
        got.append(torch.load(out))
    plain, paired = got
    assert sorted(plain) == sorted(paired)
    for k in plain:
        assert bool(torch.isfinite(plain[k]).all()), k
        assert torch.equal(plain[k], paired[k]), k
    assert float(plain["actions"].std()) > 0.1


if __name__ == "__main__":
    _child(sys.argv[1])
