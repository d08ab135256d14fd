"""GPU: the robot policy's step-1 numbers -- per-sample log-prob and value, every parameter gradient of the PPO loss, the nine scalars,
and the ReLU / max-pool decisions themselves -- against the routing-pinned fp64 reference of tests/ref64_robot.py, at the level of fp32
rounding.  Three paths through the HIP kernels (K10 + K9 + the size rules' convolutions; K11 / K12 for every hidden
convolution; K9 with the state plane and k_weighted_batch_sum), both observation shapes, clip_vloss on and off, the packed and the
unpacked loss entry; and once through ``robot_ppo.update`` itself.  Run with -s for metric, Y and ratio per tensor."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from tests import ref64_robot as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C,S", R.SHAPES, ids=["128x128x1_reference", "84x84x3_build_defined"])
@pytest.mark.parametrize("path", R.PATHS)
def test_path_matches_the_routing_pinned_fp64_step(path, C, S, monkeypatch):
    """Per path and shape: (a) every decision equals the fp64 one outside the near-tie set; (b) log-prob, value, every parameter gradient and
    the nine scalars at margin x Y; (c) exactly the kernels the path names ran.  Measured on the MI355X (DESIGN 2.5,
    profiles/robot_fp64_table.txt, the packed entry), worst ratio to Y of gradients / forward / scalars against bars of 8 / 4 / 16:
    product 2.31 / 1.30 / 1.00; hand_written_convolutions 2.80 / 1.06 / 1.00; k9_with_the_plane 1.90 / 1.11 / 1.00; the worst tensors
    are the first block's bias gradients, whose Y (1.7 - 3.5e-9) moves between runs -- up to 5.0 x Y was seen.  Before conv.hip's
    mma32x3_step the hand-written path missed the bars (third-order products lost in the accumulation, and a one-sided cut)."""
    sd, case = R.make_case(C, S)
    pol = R.gpu_policy(sd, C, S)
    calls = R.select_path(path, pol, monkeypatch.setattr, monkeypatch.setenv)
    lp, ent, v, routing, counts = R.path_evaluate(pol, case)
    assert len(routing) == R.n_decisions(sd)
    label = f"{path} {C}x{S}x{S}"
    for vmode, packed in ((O.VLOSS_CLIPPED, True), (O.VLOSS_CLIPPED, False), (O.VLOSS_RETURNS, True), (O.VLOSS_RETURNS, False)):
        ref = R.reference((C, S, 2), sd, case, routing, vmode)
        if packed:
            # (a) the masks K10 / K9 wrote and the bare ReLUs' decisions against the fp64 ones: zero disagreements outside the near-ties
            shares = R.check_routing(routing, ref["decisions"], label=label)
            print(f"\n[{label}] near-tie share per layer " + " ".join(f"{100 * s:.3f}%" for s, _ in shares)
                  + "; disagreements inside the near-tie set " + " ".join(str(n) for _, n in shares))
        # (b) forward values, gradients and scalars at margin x Y, Y = the same pinned step in plain fp32 torch on the GPU
        Y = R.gpu_yardstick((C, S, 2), sd, case, ref, vmode)
        got = R.path_step(pol, case, lp, ent, v, vmode, packed)
        R.check(got, ref, Y, f"{label} {'clip_vloss' if vmode == O.VLOSS_CLIPPED else 'returns'} {'packed' if packed else 'unpacked'}")
    R.assert_path_ran(path, counts, calls, sd, 4)


def test_update_step_1_gradient_matches_the_routing_pinned_fp64_step(monkeypatch):
    """``robot_ppo.update`` itself (product path, (1, 128, 128), 8 envs x 8 steps, 1 epoch, 2 minibatches): the flat gradient before the
    clip of optimizer step 1 and that step's scalars, on the same bars -- "step 1 runs on identical weights" extended from six scalars
    to every parameter.  The minibatch is ``np.random.RandomState(1).shuffle``'s first 32 indices (K2 is bit-exact with it)."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.robot_ppo import robot_ppo
    from aur_ppo_amd.robot_run import build_parser, params_from_args
    C, S, T, N = 1, 128, 8, 8
    p = params_from_args(build_parser().parse_args([]))
    p.update(gym_id="Synthetic-arm", num_envs=N, num_steps=T, total_timesteps=128, num_update_epochs=1, num_minibatches=2,
             do_pretraining=False, log=False, clip_vloss=True, entropy_coeff=0.01, obs_size=S, obs_channels=C)
    torch.manual_seed(2)
    agent = robot_ppo(p)
    assert agent.device.type == "cuda" and agent.minibatch_size == R.M
    cpu = R.make_policy(C, S)
    cpu.load_state_dict({k: t.cpu() for k, t in agent.policy.state_dict().items()})
    sd = {k: t.detach().clone() for k, t in cpu.state_dict().items()}
    buf, next_state, next_obs = R.make_buffers(cpu, C, S)
    for k, t in buf.items():
        getattr(agent.buffer, k).copy_(t)
    agent.seed_all(1)
    ret, adv = agent.advantages(next_state.cuda(), next_obs.cuda(), torch.zeros(N).cuda(), agent.buffer, T)
    mb = R.first_minibatch(T * N)
    case = dict(state=buf["states"].view(-1)[mb], obs=buf["observations"].view(-1, C, S, S)[mb], act=buf["actions"].view(-1, 5)[mb],
                rec=agent._rec.cpu()[mb].contiguous())
    hyper = dict(clip=p["clip_coeff"], ent_coef=p["entropy_coeff"], vf_coef=p["value_coeff"])
    moved = R.make_records_safe(sd, case, hyper)          # the records the update reads, clear of the loss's branches
    agent._rec[mb.cuda()] = case["rec"].cuda()
    grabbed, packed_calls = [], []
    real_step, real_loss = agent._clip_and_step, H.ppo_loss_packed
    monkeypatch.setattr(agent, "_clip_and_step", lambda *a, **k: (grabbed or grabbed.append(agent.bucket.flat_grad.detach().clone()), real_step(*a, **k))[1])
    monkeypatch.setattr(H, "ppo_loss_packed", lambda *a, **k: (packed_calls.append(1), real_loss(*a, **k))[1])
    with R.capture_routing(agent.policy) as (rec, counts):
        agent.update(agent.buffer.flatten(ret, adv), 1, agent.batch_size, agent.minibatch_size, [])
    n = R.n_decisions(sd)
    assert len(rec) == 2 * n and len(packed_calls) == 2 and len(grabbed) == 1 and counts["K10"] == 4 and counts["K9"] >= 2 * 2 * 3
    routing = rec[:n]
    vmode = O.VLOSS_CLIPPED
    ref = R.reference(("update", C, S), sd, case, routing, vmode, hyper)
    shares = R.check_routing(routing, ref["decisions"], label="update")
    print(f"\n[update] records moved {moved}; near-tie share per layer " + " ".join(f"{100 * s:.3f}%" for s, _ in shares))
    Y = R.gpu_yardstick(("update", C, S), sd, case, ref, vmode, hyper)
    names = {id(q): k for k, q in agent.policy.named_parameters()}
    grads, off = {}, 0
    for q in agent.bucket.params:
        grads[names[id(q)]] = grabbed[0][off:off + q.numel()].view_as(q)
        off += q.numel()
    for k in grads:
        if k not in ref["names"]:
            assert not bool(grads[k].any()), f"{k}: a parameter outside the actor and the critic received a gradient"
    R.check(dict(grads=grads, scalars=torch.from_numpy(np.asarray(agent._last_scalars[0]))), ref, Y, "robot_ppo.update, optimizer step 1")
