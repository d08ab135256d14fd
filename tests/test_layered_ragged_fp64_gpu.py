"""GPU: the layered PPO step and the layered rollout step at state widths that are no multiple of 16 (Hopper's 11, HalfCheetah's 17,
Humanoid's 376, ...: ``mlp_layered_layout(..., any_state=True)``, layer 0's products on k_linear_tail / k_linear_wgrad_tail), against
the fp64 reference of tests/ref64.py used as it is.

T1  the step: the body of tests/test_layered_fp64_gpu.py::test_layered_step_matches_fp64 -- reference, metric, GPU yardstick and the
    bars MARGIN / MARGIN_TINY_M / MARGIN_SCALARS unchanged, a second launch gives the same bits, nothing past ``n_params`` is written.
T2  the rollout step: the body of tests/test_layered_act_fp64_gpu.py::test_layered_act_matches_fp64 -- guarded outputs, a repeat,
    prepared weights, value-only; bar MARGIN, every Categorical index equal.
T3  the rollout's log-prob and value are the update's: old_kl, kl and clipfrac exactly 0, so the plain and the ROWS tail builds give a
    row the same bits wherever it sits.
tests/test_layered_ragged_host.py shows on the CPU that a correct fp32 computation meets the bars at every case's shape."""
import numpy as np
import pytest
import torch

from tests import layered_act_cases as LA
from tests import layered_ragged_cases as LR
from tests import ref64 as R

pytestmark = pytest.mark.gpu

GUARD = 64          # floats of NaN either side of every output
SHIFT = 3           # the outputs start 3 floats past a 16-byte boundary: 4-byte aligned, not 16


def _policy(hidden, layers, D, A, cont, sd=None, seed=0):
    """The project's actor_critic on the GPU (the case's weights, or seeded ones moved off their initialisation), its flat bucket and
    its layered layout, taken through ``any_state=True``."""
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
    lay = H.mlp_layered_layout(pol, bucket, any_state=True)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (D, A, hidden, layers)
    if sd is not None:
        assert [n for n, _ in pol.named_parameters()] == R.param_names(R.make_net(sd)), "FlatBucket order"
    return H, pol, bucket, lay


class _Guarded:
    """An (n,) or (n, w) output as a view into a NaN-filled buffer: GUARD floats, SHIFT more, the view, GUARD floats."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((GUARD + SHIFT + n + GUARD + 4,), float("nan"), device="cuda")
        base = (-self.buf.data_ptr() % 16) // 4         # floats to the next 16-byte boundary
        self.lo = base + GUARD + SHIFT
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.view.data_ptr() % 16 != 0 and self.view.data_ptr() % 4 == 0 and self.view.is_contiguous()
        self.n = n

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


# ---------------------------------------------------------------------------------- T1: the step
@pytest.mark.parametrize("c", LR.STEP_CASES, ids=LR.STEP_IDS)
def test_layered_step_matches_fp64_at_a_ragged_state(c):
    """Scalars and every gradient tensor of one step, element by element on the scale of the terms behind each element; a second
    launch gives the same bits; nothing past ``n_params`` is written."""
    data = R.build_case(c)
    ref = R.reference_step(c, data)
    data["ref"] = ref
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    H, _pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
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
    R.check_step(c, sc, g[:n], ref, Y, Ys, "layered, ragged D: k_linear_tail + K13 k_head_ppo")


# ---------------------------------------------------------------------------------- T2: the rollout step
@pytest.mark.parametrize("c", LR.ACT_CASES, ids=LR.ACT_IDS)
def test_layered_act_matches_fp64_at_a_ragged_state(c):
    data = LA.build(c)
    ref = data["ref"]
    Y, y = LA.yardstick(c, data, "cuda")
    H, pol, bucket, lay = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    N = c.M
    obs, noise = data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous()

    def run(wop=None):
        ga, gl, gv = _Guarded(*((N, c.A) if c.cont else (N,))), _Guarded(N), _Guarded(N)
        a, lp, v = H.mlp_layered_act(obs, noise, bucket.flat_param, lay, ga.view, gl.view, gv.view, wop=wop)
        torch.cuda.synchronize()
        assert a is ga.view and lp is gl.view and v is gv.view
        assert ga.guards_intact() and gl.guards_intact() and gv.guards_intact(), "a guard was written"       # (a)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(v).all())
        return a.clone(), lp.clone(), v.clone()

    a, lp, v = run()
    if not c.cont:
        assert torch.equal(a.long().cpu(), ref["action"]), int((a.long().cpu() != ref["action"]).sum())
    m = LA.metrics(c, ref, v, a, lp)
    print(f"\n[layered act, ragged D: k_linear_tail + K14 k_head_act] {R.case_id(c)}: "
          + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items()) + f" (Y {Y:.3e}; moved {data['moved']})")
    for n, x in m.items():
        assert x <= R.MARGIN * Y, (n, x, Y, x / Y)
    for got, first in zip(run(), (a, lp, v)):                                                                # (b)
        assert torch.equal(got, first), "two calls differ"
    for got, first in zip(run(H.mlp_layered_prepare(bucket.flat_param, lay)), (a, lp, v)):                      # (c)
        assert torch.equal(got, first), "prepared weights change the result"
    gv = _Guarded(N)                                                                                         # (d)
    a0, lp0, v0 = H.mlp_layered_act(obs, None, bucket.flat_param, lay, value=gv.view)
    torch.cuda.synchronize()
    assert a0 is None and lp0 is None and torch.equal(v0, v) and gv.guards_intact()


# ---------------------------------------------------------------------------------- T3: the rollout's log-prob is the update's
@pytest.mark.parametrize("hidden,layers,D,A,cont,N,M,packed", [(256, 2, 17, 6, True, 513, 300, False), (160, 3, 11, 3, True, 257, 100, True)],
                         ids=["2x256-D17", "3x160-D11-packed"])
def test_the_rollouts_logp_and_value_are_the_updates_at_a_ragged_state(hidden, layers, D, A, cont, N, M, packed):
    """``mlp_layered_act`` over N rows (k_linear_tail, plain addressing), then ``mlp_layered_step`` over a permutation slice of them
    (k_linear_tail through the index) with old_logp / old_v from the rollout: the ratio is exp(0) for every sample, so old_kl, kl and
    clipfrac are exactly 0."""
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
    sc = H.mlp_layered_step(obs, acts, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED).cpu()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(grad[:lay["n_params"]]).all())
    print(f"\n{layers} x {hidden}, D {D}: old_kl {float(sc[H.S_OLD_KL])!r}, kl {float(sc[H.S_KL])!r}, clipfrac {float(sc[H.S_CLIPFRAC])!r}")
    assert float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0
    # the value took part too: the clipped value loss sees v - old_v == 0, so vl = 0.5 * mean((v - ret)^2) exactly as un-clipped
    sc_u = H.mlp_layered_step(obs, acts, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_RETURNS).cpu()
    assert float(sc_u[H.S_VL]) == float(sc[H.S_VL])
