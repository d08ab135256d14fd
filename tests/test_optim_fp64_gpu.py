"""GPU: the five launches that write the parameters -- K6 (``grad_norm_clip_``), K6b (``clip_adam_``), ``mlp_ppo_apply``,
``mlp_ppo_apply_parts`` and the chained tail of ``mlp_ppo_minibatch`` (K7 and K7w) -- against the fp64 clip + Adam of
tests/ref64_optim.py, at the level of fp32 rounding.

Every check is ``metric <= margin x Y``: the metric is the error against fp64 over the sum of the absolute terms behind the number, Y is
what ``clip_grad_norm_`` + single-tensor ``torch.optim.Adam`` in fp32 on the GPU lose on the same case and metric (floored at 2^-24), and
the margins (``ref64_optim.MARGINS``) come from a second correct fp32 formulation on the CPU (tests/test_optim_fp64_host.py, which also
shows the wrong formulas these bars reject).  No element is excluded and nothing is skipped.  ``-s`` prints every figure."""
import math

import numpy as np
import pytest
import torch

from tests import ref64 as R64
from tests import ref64_optim as R

pytestmark = pytest.mark.gpu


def _judge(label, case, got, quantities=R.QUANTITIES):
    ref = R.reference_of(case)
    Y, _ = R.yardstick(case, ref, "cuda")
    return R.check(label, got, ref, Y, quantities=quantities)


# ---------------------------------------------------------------------------------- K6 / K6b on a flat bucket
@pytest.mark.parametrize("kw", R.K6_CASES, ids=[f"n{kw['n']}-{kw['gscale']}" for kw in R.K6_CASES])
def test_grad_norm_clip_matches_fp64(kw):
    case = R.build(**kw)
    _judge("K6 " + case["id"], case, R.run_k6(case), ("norm", "gc"))


@pytest.mark.parametrize("kw", R.K6B_CASES, ids=[f"n{kw['n']}-clip{kw['clip_n']}-{kw['gscale']}-{kw['state']}-t{kw['t']}-lr{kw['lr']:g}-p{kw['p0_kind']}"
                                                 for kw in R.K6B_CASES])
def test_clip_adam_matches_fp64(kw):
    """Norm, the clipped gradient left in g, m, v, p, and the step count (exactly t)."""
    case = R.build(**kw)
    got, step = R.run_k6b(case)
    assert step == case["t"]
    _judge("K6b " + case["id"], case, got)


# ---------------------------------------------------------------------------------- k_adam_chain behind mlp_ppo_apply / mlp_ppo_apply_parts
def _policy(pol):
    D, A, cont = pol
    c = R64._mk("k7", 64, 2, D, A, cont, 1, False, 0)
    sd = R64.make_policy_sd(64, 2, D, A, cont, np.random.RandomState(D * 31 + A))
    _pol, bucket, lay = R64.gpu_policy(c, sd)
    assert lay["n_params"] == R.policy_n_params(*pol)
    return lay


_POL_IDS = [f"D{D}-A{A}-{'gauss' if cont else 'cat'}" for D, A, cont in R.APPLY_POLICIES]


@pytest.mark.parametrize("pol", R.APPLY_POLICIES, ids=_POL_IDS)
def test_apply_matches_fp64_and_leaves_the_gradient_alone(pol):
    """``mlp_ppo_apply`` forms the norm of ``g * grad_scale`` itself (16-byte loads plus a tail) and must hand ``flat_grad`` back bit
    for bit; the step count is the caller's.  Six cases per policy; the last one again with the gradient a view that starts 4 bytes
    into its buffer (no 16-byte loads: the n4 = 0 path)."""
    lay = _policy(pol)
    n = lay["n_params"]
    cases = [R.build(n=n, **kw) for kw in R.apply_cases(pol)]
    for case, misalign in [(c, False) for c in cases] + [(cases[-1], True)]:
        got, step, g_bits = R.run_apply(case, lay, misalign=misalign)
        assert step == case["t"]
        assert np.array_equal(g_bits, case["g"].view(np.int32)), "mlp_ppo_apply changed flat_grad"
        _judge(f"apply{' (g misaligned)' if misalign else ''} " + case["id"], case, got, ("norm", "m", "v", "p"))


@pytest.mark.parametrize("pol", R.APPLY_POLICIES, ids=_POL_IDS)
def test_apply_parts_matches_fp64(pol):
    """``mlp_ppo_apply_parts`` with the clip's partial sums built on the host in fp64 from the gradient (no second process): 1, 255,
    257 and ``aurppo_p2p_parts(n)`` sums, and once ``aurppo_p2p_parts(n)`` entries of which all but three are 0."""
    from aur_ppo_amd import _lib
    lay = _policy(pol)
    n = lay["n_params"]
    p2p = int(_lib.load().aurppo_p2p_parts(n))
    assert p2p > 3
    for kw, parts in R.parts_cases(pol):
        case = R.build(n=n, **kw)
        n_part = p2p if isinstance(parts, str) else parts
        sq = R.host_sq_parts(case["g"], n_part, sparse=parts == "p2p-sparse")
        assert sq.size == n_part and (parts != "p2p-sparse" or int((sq != 0).sum()) == 3)
        got, step, _ = R.run_apply(case, lay, parts=sq)
        assert step == case["t"]
        _judge(f"apply_parts[{parts}: {n_part}] " + case["id"], case, got)


# ---------------------------------------------------------------------------------- the chained tail as the trainer runs it
_TAIL_SHAPES = [R64._mk("k7", 64, 2, 64, 6, True, 300, True, 1),          # k_mlp_step3 / k_mlp_step2 -> k_mlp_reduce_x4 -> k_adam_chain
                R64._mk("k7w", 64, 1, 64, 6, True, 300, True, 1), R64._mk("k7w", 32, 3, 5, 4, False, 300, True, 1),       # K7w id 1
                R64._mk("k7w", 128, 3, 128, 16, True, 300, True, 1),      # ids 3 / 2: the largest bucket (128 workgroups, four elements per thread)
                R64._mk("k7w", 100, 2, 100, 6, True, 300, True, 1), R64._mk("k7w", 65, 1, 1, 3, False, 300, True, 1)]
_TAIL = [(c, k) for c in _TAIL_SHAPES for k in R64.kernels_for(c)]
_TAIL_IDS = [f"{k.name}-{R64.case_id(c)}" for c, k in _TAIL]
_DATA = {}


def _data(c):
    if c not in _DATA:
        d = R64.build_case(c)
        d["gpu"] = R64.gpu_inputs(c, d)
        rs = np.random.RandomState(c.seed + 5)
        d["idx1"] = torch.from_numpy(rs.permutation(d["obs"].shape[0])[:200].astype(np.int32)).cuda()
        del d["net64"]
        _DATA[c] = d
    return _DATA[c]


def _minibatch(H, c, d, bucket, lay, idx, g, m_, v_, lr, t, max_norm, sc, norm, next_idx=None, chained=False, norm_adv=None):
    obs, act, rec, _ = d["gpu"]
    H.mlp_ppo_minibatch(obs, act, rec, idx, bucket.flat_param, lay, g, R64.HYPER["clip"], R64.HYPER["ent_coef"], R64.HYPER["vf_coef"],
                        c.norm_adv if norm_adv is None else norm_adv, c.vmode, sc, m_, v_, lr, t, max_norm, R.BETAS, R.EPS, norm,
                        next_idx=next_idx, chained=chained)


_TAIL_T = [(0, 3e-4), (999, 1.0)]


def tail_runs(c, k, t0, lr, setenv):
    """The three runs of one (shape, kernel, step count): yields (label, case, outputs) after asserting what needs no reference."""
    from aur_ppo_amd import hip_ops as H
    d = _data(c)
    label = R64.select_kernel(c, k, 1, setenv)
    _pol, bucket, lay = R64.gpu_policy(c, d["sd"])
    n, nb = lay["n_params"], bucket.flat_param.numel()
    p_init = bucket.flat_param.detach().clone()
    _sc, g0 = R64.kernel_step(c, d, (_pol, bucket, lay))
    torch.cuda.synchronize()
    g0 = g0.cpu().numpy().copy()
    norm0 = math.sqrt(float(np.sum(g0.astype(np.float64) ** 2)))
    rs = np.random.RandomState(c.seed + t0)
    s = norm0 / math.sqrt(n)
    m0, v0 = 0.3 * s * rs.standard_normal(n), 0.5 * s * s * (0.25 + rs.random_sample(n))
    cold = rs.random_sample(n) < 0.05
    m0[cold], v0[cold] = 0.0, 0.0
    m0, v0 = m0.astype(np.float32), v0.astype(np.float32)
    pad = torch.arange(nb - n, device="cuda", dtype=torch.float32) + 0.5
    for which, max_norm in (("inactive", 1e9), ("edge", R.f32(norm0 / 1.5)), ("active", R.f32(norm0 / 100))):
        with torch.no_grad():
            bucket.flat_param.copy_(p_init)
        g, m_, v_ = (torch.zeros(nb, device="cuda") for _ in range(3))
        m_[:n], v_[:n] = torch.from_numpy(m0).cuda(), torch.from_numpy(v0).cuda()
        m_[n:], v_[n:], g[n:] = pad, pad, pad
        lr_d, t = torch.tensor([lr], device="cuda", dtype=torch.float32), torch.tensor([float(t0)], device="cuda")
        sc, norm = torch.zeros(9, device="cuda"), torch.full((1,), float("nan"), device="cuda")
        _minibatch(H, c, d, bucket, lay, d["gpu"][3], g, m_, v_, lr_d, t, max_norm, sc, norm)
        torch.cuda.synchronize()
        assert float(t) == t0 + 1
        assert torch.equal(m_[n:], pad) and torch.equal(v_[n:], pad) and torch.equal(g[n:], pad), "padding past n_params was written"
        if which == "inactive":
            assert np.array_equal(g[:n].cpu().numpy().view(np.int32), g0.view(np.int32)), "mlp_ppo_step's gradient is not the chained call's"
        case = dict(n=n, clip_n=n, t=t0 + 1, lr=lr, max_norm=max_norm, grad_scale=1.0, betas=R.BETAS, eps=R.EPS, p0=p_init[:n].cpu().numpy(),
                    g=g0, m0=m0, v0=v0, id=f"{R64.case_id(c)}-t{t0 + 1}-lr{lr:g}-{which}")
        R.assert_input_condition(case)
        yield f"{label} tail", case, R.outputs(norm, g, m_, v_, bucket.flat_param.detach(), n)


@pytest.mark.parametrize("t0,lr", _TAIL_T, ids=["t1", "t1000-lr1"])
@pytest.mark.parametrize("c,k", _TAIL, ids=_TAIL_IDS)
def test_minibatch_tail_matches_the_fp64_optimizer_on_the_gradient_it_was_given(c, k, t0, lr, monkeypatch):
    """``mlp_ppo_minibatch`` on margin-safe data with static tiles, warm moments, M = 300.  The unclipped gradient is read first with
    ``mlp_ppo_step`` on the same inputs (bit-identical under static tiles: asserted on the run with max_norm = 1e9); then three runs
    with max_norm = 1e9, norm / 1.5 (the edge regime) and norm / 100, each held to the fp64 clip + Adam of THAT fp32 gradient: norm, the
    gradient the call leaves, m, v, p, the step count, and the padding past n_params untouched."""
    for label, case, got in tail_runs(c, k, t0, lr, monkeypatch.setenv):
        _judge(label + " " + case["id"], case, got)


# ---------------------------------------------------------------------------------- what the optimizer launch hands over
def _adv_scalars_check(label, sc, adv):
    """adv_mean / adv_std of the slice against fp64, over mean |adv| and the root mean square, at MARGIN_SCALARS x (fp32 torch's own
    error on the GPU, at least one fp32 ulp of the scale) -- ref64's bar for the nine scalars."""
    a64 = adv.double().cpu()
    want = (float(a64.mean()), float(a64.std()))
    scale = (float(a64.abs().mean()), float((a64 * a64).mean().sqrt()))
    torch32 = (float(adv.mean()), float(adv.std()))
    got = (float(sc[7]), float(sc[8]))
    Y = max(max(abs(a - b) / s for a, b, s in zip(torch32, want, scale)), R64.ULP32)
    ms = [abs(a - b) / s for a, b, s in zip(got, want, scale)]
    print(f"\n[{label}] adv_mean {ms[0]:.3e}, adv_std {ms[1]:.3e} against Y {Y:.3e} (margin {R64.MARGIN_SCALARS:g})")
    assert max(ms) <= R64.MARGIN_SCALARS * Y, (label, ms, Y)


_HAND = [(c, k, "minibatch") for c, k in _TAIL] + [(c, k, "grad+apply") for c, k in _TAIL if c.kind == "k7"]


@pytest.mark.parametrize("c,k,mode", _HAND, ids=[f"{k.name}-{mode}-{R64.case_id(c)}" for c, k, mode in _HAND])
def test_the_next_chained_step_sees_the_updated_parameters_bit_for_bit(c, k, mode, monkeypatch):
    """After a minibatch that named ``next_idx``, the chained step reads operand copies and statistics the optimizer launch prepared.
    With static tiles and ``norm_adv=False`` (the advantage statistics then only reach the two reported scalars) its gradient must
    equal, bit for bit, a fresh ``mlp_ppo_step`` at the updated parameters on the same slice; the two advantage scalars are held to
    fp64."""
    from aur_ppo_amd import hip_ops as H
    d = _data(c)
    label = R64.select_kernel(c, k, 1, monkeypatch.setenv)
    _pol, bucket, lay = R64.gpu_policy(c, d["sd"])
    n, nb = lay["n_params"], bucket.flat_param.numel()
    obs, act, rec, idx0 = d["gpu"]
    idx1 = d["idx1"]
    p_before = bucket.flat_param.detach().clone()
    g, m_, v_ = (torch.zeros(nb, device="cuda") for _ in range(3))
    lr, t = torch.tensor([3e-3], device="cuda"), torch.zeros(1, device="cuda")
    sc, norm = torch.zeros(2, 9, device="cuda"), torch.zeros(2, device="cuda")
    hy = (R64.HYPER["clip"], R64.HYPER["ent_coef"], R64.HYPER["vf_coef"], False, c.vmode)
    if mode == "minibatch":
        _minibatch(H, c, d, bucket, lay, idx0, g, m_, v_, lr, t, 0.5, sc[0], norm[0:1], next_idx=idx1, norm_adv=False)
        torch.cuda.synchronize()
        p1 = bucket.flat_param.detach().clone()
        _minibatch(H, c, d, bucket, lay, idx1, g, m_, v_, lr, t, 1e9, sc[1], norm[1:2], chained=True, norm_adv=False)
    else:
        H.mlp_ppo_grad(obs, act, rec, idx0, bucket.flat_param, lay, g, *hy, sc[0], t, chained=False)
        H.mlp_ppo_apply(bucket.flat_param, g, m_, v_, lay, lr, t, 0.5, R.BETAS, R.EPS, norm[0:1], rec=rec, next_idx=idx1)
        torch.cuda.synchronize()
        p1 = bucket.flat_param.detach().clone()
        H.mlp_ppo_grad(obs, act, rec, idx1, bucket.flat_param, lay, g, *hy, sc[1], t, chained=True)
    torch.cuda.synchronize()
    chained_g = g[:n].clone()             # max_norm = 1e9: the clip leaves the gradient as the step wrote it
    assert float(t) == 2 and float((p1[:n] - p_before[:n]).abs().max()) > 1e-4      # the first call did move the parameters
    fresh_g = torch.full_like(g, float("nan"))
    fresh_sc = H.mlp_ppo_step(obs, act, rec, idx1, p1, lay, fresh_g, *hy)
    torch.cuda.synchronize()
    diff = int((chained_g.view(torch.int32) != fresh_g[:n].view(torch.int32)).sum())
    print(f"\n[{label} {mode}] {R64.case_id(c)}: {diff} of {n} gradient elements differ from a fresh step at the updated parameters")
    assert diff == 0
    assert torch.equal(sc[1][:7], fresh_sc[:7]), (sc[1], fresh_sc)
    _adv_scalars_check(f"{label} {mode} chained", sc[1], rec[idx1.long(), 1])
    _adv_scalars_check(f"{label} {mode} fresh", fresh_sc, rec[idx1.long(), 1])


# ---------------------------------------------------------------------------------- non-finite gradients
def _nonfinite_case(n, clip_n, bad, at):
    case = R.build(n, "active", "warm", 10, 3e-4, "random", clip_n, 1.0, R.case_seed(n, 3, 9))
    case["g"] = case["g"].copy()
    case["g"][at] = bad
    case["id"] += f"-g[{at}]={bad}"
    return case


def _judge_nonfinite(label, case, got, quantities):
    """The class (finite / NaN / +inf / -inf) of every element and of the norm must be what fp32 torch produces for the case; the
    elements torch leaves finite meet the bars."""
    with np.errstate(all="ignore"):
        ref = R.reference_of(case)
    tr = R.torch_run(case, "cuda")
    for q in quantities:
        assert np.array_equal(R.classes(got[q]), R.classes(tr[q])), (label, q, "class differs from fp32 torch's")
    elem = [q for q in quantities if q != "norm"]
    mask = np.logical_and.reduce([R.classes(tr[q]) == 0 for q in elem])
    assert 0 < int(mask.sum())
    judged = elem + (["norm"] if math.isfinite(tr["norm"]) else [])
    Y = {q: max(x, R.ULP32) for q, x in R.metrics(tr, ref, mask, judged).items()}
    R.check(label, got, ref, Y, mask, judged)
    return tr, mask


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_clip_adam_with_a_non_finite_gradient_element(bad):
    """K6b, n = 1025, clip_n = n // 3 with the bad element inside the clipped slice.  NaN: everything clipped becomes NaN, as
    ``clip_grad_norm_`` does, and the elements past clip_n stay finite.  +inf: coef = 0, that element is NaN, the other clipped
    ones are 0."""
    n = 1025
    case = _nonfinite_case(n, n // 3, bad, 7)
    got, step = R.run_k6b(case)
    assert step == case["t"]
    tr, mask = _judge_nonfinite(f"K6b g[7]={bad}", case, got, ("norm", "gc", "m", "v", "p"))
    assert int(mask.sum()) == (n - n // 3 if math.isnan(bad) else n - 1)
    if math.isinf(bad):
        sl = np.arange(n // 3) != 7
        assert math.isinf(got["norm"]) and np.isnan(got["gc"][7]) and np.all(got["gc"][:n // 3][sl] == 0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_apply_with_a_non_finite_gradient_element(bad):
    """``mlp_ppo_apply`` on the smallest 2 x 64 bucket (D 1, Categorical, A 4: its n is the policy's, 8901), grad_scale 1/2."""
    pol = (1, 4, False)
    lay = _policy(pol)
    n = lay["n_params"]
    case = _nonfinite_case(n, n, bad, n - 2)
    case["grad_scale"] = 0.5
    got, step, g_bits = R.run_apply(case, lay)
    assert step == case["t"] and np.array_equal(g_bits, case["g"].view(np.int32))
    if math.isnan(bad):          # nothing is left finite: classes only
        tr = R.torch_run(case, "cuda")
        for q in ("norm", "m", "v", "p"):
            assert np.array_equal(R.classes(got[q]), R.classes(tr[q])), q
        assert math.isnan(got["norm"]) and np.all(np.isnan(got["p"]))
    else:
        _tr, mask = _judge_nonfinite(f"apply g[{n - 2}]={bad}", case, got, ("norm", "m", "v", "p"))
        assert int(mask.sum()) == n - 1
