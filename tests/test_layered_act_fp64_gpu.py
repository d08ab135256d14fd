"""GPU: the layered rollout step (hip_ops.mlp_layered_act: per net the hidden layers on k_linear from operand copies prepared once,
then K14 k_head_act -- csrc/head.hip) for the MLP policies wider than the fused kernels.

T1  against the fp64 reference of tests/ref64.py used as it is (``act_reference``, the metric and the bar ``MARGIN`` of
    test_mlp_fp64_gpu.py::test_act_kernel_matches_fp64; Y: the same formulas in fp32 torch on the GPU, floored at one ulp; the
    Categorical index EQUAL for every row after ``safe_uniform``; nothing excluded), with outputs that are views into NaN-filled
    buffers at a 4-byte-aligned offset, a repeat, a prepared-weights call and the value-only mode.
T2  the log-prob and value the rollout step stores are bit for bit the ones the layered update step forms from the stored action at
    the same parameters: ``old_kl``, ``kl`` and ``clipfrac`` of ``mlp_layered_step`` over a slice of those rows are exactly 0.
T3  K14 alone on random activations against fp32 torch, and its shape limits through the C ABI.
tests/test_layered_act_host.py shows on the CPU that a correct fp32 computation meets T1's bar at every case's shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import layered_act_cases as LA
from tests import ref64 as R

pytestmark = pytest.mark.gpu

GUARD = 64          # floats of NaN either side of every output
SHIFT = 3           # the outputs start 3 floats past a 16-byte boundary: 4-byte aligned, not 16


def _policy(hidden, layers, D, A, cont, sd=None, seed=0):
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
    return H, pol, bucket


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


@pytest.mark.parametrize("c", LA.CASES, ids=LA.IDS)
def test_layered_act_matches_fp64(c):
    data = LA.build(c)
    ref = data["ref"]
    Y, y = LA.yardstick(c, data, "cuda")
    H, pol, bucket = _policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    assert H.mlp_layout(pol, bucket) is None
    lay = H.mlp_layered_layout(pol, bucket)
    assert lay is not None and (lay["D"], lay["A"], lay["hidden"], lay["num_layers"]) == (c.D, c.A, c.hidden, c.layers)
    assert [n for n, _ in pol.named_parameters()] == R.param_names(R.make_net(data["sd"])), "FlatBucket order"
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
    print(f"\n[layered act: k_linear + K14 k_head_act] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items())
          + f" (Y {Y:.3e}; moved {data['moved']})")
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


# ---------------------------------------------------------------------------------- T2: the rollout's log-prob is the update's
@pytest.mark.parametrize("hidden,layers,D,A,cont,N,M,packed", [(256, 2, 64, 6, True, 513, 300, False), (1024, 1, 64, 16, False, 65, 65, False),
                                                               (160, 3, 144, 12, True, 257, 100, True)],
                         ids=["2x256-gauss", "1x1024-cat", "3x160-gauss-packed"])
def test_the_rollouts_logp_and_value_are_the_updates(hidden, layers, D, A, cont, N, M, packed):
    """``mlp_layered_act`` over N rows, then ``mlp_layered_step`` over a permutation slice of them with old_logp / old_v from the
    rollout: the ratio is exp(0) for every sample, so old_kl, kl and clipfrac are exactly 0 -- K14's head order and distribution
    expressions are K13's, and a row's hidden activations do not depend on where the row sits."""
    H, pol, bucket = _policy(hidden, layers, D, A, cont, seed=hidden + N)
    lay = H.mlp_layered_layout(pol, bucket)
    assert lay is not None
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
    print(f"\n{layers} x {hidden}: old_kl {float(sc[H.S_OLD_KL])!r}, kl {float(sc[H.S_KL])!r}, clipfrac {float(sc[H.S_CLIPFRAC])!r}")
    assert float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0
    # the value took part too: the clipped value loss sees v - old_v == 0, so vl = 0.5 * mean((v - ret)^2) exactly as un-clipped
    sc_u = H.mlp_layered_step(obs, acts, rec, idx, bucket.flat_param, lay, grad, 0.2, 0.01, 0.5, True, H.VLOSS_RETURNS).cpu()
    assert float(sc_u[H.S_VL]) == float(sc[H.S_VL])


# ---------------------------------------------------------------------------------- T3: K14 alone
@pytest.mark.parametrize("cont", [True, False], ids=["gauss", "cat"])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("Hd", [32, 1024])
def test_head_act_kernel_matches_torch_formulas(Hd, N, cont):
    """Tolerances of tests/test_mlp_wide.py::test_wide_act_kernel_matches_torch_formulas."""
    A, D = 6, 16
    H, pol, bucket = _policy(Hd, 1, D, A, cont, seed=Hd + N)
    seq, n, _D, _A, _cont, NL, _Hd = H._mlp_structure(pol, bucket)
    lay = dict(offsets=seq, n_params=n, D=D, A=A, continuous=cont, hidden=Hd, num_layers=NL, layered=True)
    g = torch.Generator(device="cuda").manual_seed(Hd * 3 + N)
    hA = torch.tanh(torch.randn(N, Hd, device="cuda", generator=g))
    hC = torch.tanh(torch.randn(N, Hd, device="cuda", generator=g))
    with torch.no_grad():
        v_ref = pol.critic.net[2](hC).view(-1)
        out = pol.actor.net[2](hA)
        if cont:
            noise = torch.randn(N, A, device="cuda", generator=g)
            std = pol.actor_logstd.exp().expand_as(out)
            a_ref = out + std * noise
            lp_ref = torch.distributions.Normal(out, std).log_prob(a_ref).sum(1)
        else:
            noise = torch.rand(N, device="cuda", generator=g)
            cdf = torch.softmax(out, 1).cumsum(1)
            a_ref = (noise[:, None] >= cdf).sum(1).clamp(max=A - 1).float()
            lp_ref = torch.log_softmax(out, 1).gather(1, a_ref.long()[:, None])[:, 0]
    a, lp, v = H.head_act(hA, hC, noise, bucket.flat_param, lay)
    torch.cuda.synchronize()
    np.testing.assert_allclose(v.cpu().numpy(), v_ref.cpu().numpy(), rtol=2e-5, atol=1e-5)
    if cont:
        np.testing.assert_allclose(a.cpu().numpy(), a_ref.cpu().numpy(), rtol=2e-5, atol=1e-5)
        np.testing.assert_allclose(lp.cpu().numpy(), lp_ref.cpu().numpy(), rtol=2e-5, atol=2e-5)
    else:
        same = (a == a_ref)          # a draw within rounding of a CDF boundary may land on either side
        assert float(same.float().mean()) >= 0.99
        np.testing.assert_allclose(lp[same].cpu().numpy(), lp_ref[same].cpu().numpy(), rtol=2e-5, atol=2e-5)
    a0, lp0, v0 = H.head_act(None, hC, None, bucket.flat_param, lay)                  # value only
    assert a0 is None and lp0 is None and torch.equal(v0, v)


def test_head_act_refuses_shapes_outside_its_limits():
    """H a multiple of 32 in 32..1024, A in 1..16 (Categorical 2..16), N > 0: AURPPO_ESHAPE through the C ABI, before any launch."""
    from aur_ppo_amd import _lib
    H, pol, bucket = _policy(32, 1, 16, 6, True)
    lib = _lib.load()
    ESHAPE = -2          # include/aurppo.h
    h = torch.zeros(4, 2048, device="cuda")
    noise, out = torch.zeros(4, 16, device="cuda"), torch.zeros(4, 16, device="cuda")
    lay = (C.c_int * 5)(0, 0, 0, 0, 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rc(N, Hd, A, cont):
        return lib.aurppo_head_act_f32(p(h), p(h), p(noise), N, Hd, A, cont, p(bucket.flat_param), lay, 1 << 30, p(out), p(out), p(out), st)
    for N, Hd, A, cont in [(4, 16, 6, 1), (4, 48, 6, 1), (4, 1056, 6, 1), (4, 0, 6, 1), (4, 64, 0, 1), (4, 64, 17, 1), (4, 64, 1, 0), (0, 64, 6, 1)]:
        assert rc(N, Hd, A, cont) == ESHAPE, (N, Hd, A, cont)
    torch.cuda.synchronize()
