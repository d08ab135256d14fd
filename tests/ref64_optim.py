"""fp64 reference of the step every optimizer launch ends in -- global-norm clip over the first ``clip_n`` elements of a flat gradient,
then torch's single-tensor Adam over all of it (csrc/clip.hip's header comment, csrc/adam_math.h) -- with the metric the kernels are
judged on, the yardstick, a second correct fp32 formulation with its wrong variants, and the inputs.  A plain helper module (no tests in
it); DESIGN's parity section derives the bars.

What is here
  * ``reference``: float64 numpy on the fp32 inputs as given.  ``t`` is the step count the update uses (after the increment).  The
    hyper-parameters are the fp32 roundings the kernels and fp32 torch both use; ``rounded=False`` turns those off, so that a host test
    can hold the reference to torch's own float64 optimizer.
  * ``metrics``: every number over the sum of the absolute terms behind it, from the fp64 run.  No floors, no exclusions: where the scale
    is zero the value must be exactly the reference's.
  * ``torch_run``: ``clip_grad_norm_(foreach=False)`` on the slice + ``torch.optim.Adam(foreach=False, fused=False, capturable=False)``
    with the state injected.  In float32 it is the YARDSTICK Y (``yardstick``: its metric, floored at 2^-24); in float64 the host
    test's witness for ``reference``.
  * ``replay_fp32``: adam_math.h's operation order in numpy float32, with ``mutant=`` for the wrong variants of ``MUTANTS``.
  * ``build``: the inputs of a case from ``np.random.RandomState``, with the condition on them asserted in fp64.
  * ``check``: the bars of one launch, printed then asserted.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

ULP32 = 2.0 ** -24
BETAS, EPS, MAX_NORM = (0.9, 0.999), 1e-5, 0.5
QUANTITIES = ("norm", "gc", "m", "v", "p")
# metric <= margin * Y per quantity.  The worst ratio of ``replay_fp32`` against the CPU's Y over the regime grid, rounded up to the next
# power of two (tests/test_optim_fp64_host.py re-measures and prints them; DESIGN 2.2 keeps the figures): not taken from the kernels.
MARGINS = dict(norm=2.0, gc=2.0, m=4.0, v=4.0, p=4.0)
F32_TINY, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)

GSCALES = ("inactive", "active", "edge")          # gradient scale 1e-3 / 10 / rescaled to a clipped norm of 1.5 * max_norm
STATES = (("zero", 1), ("warm", 1), ("warm", 2), ("warm", 10), ("warm", 1000), ("warm", 100000))      # (state, t)
LRS = (3e-4, 1.0)
P0S = ("random", "zero")
GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0)


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ reference
def _hyper(max_norm, grad_scale, betas, eps, rounded):
    r = f32 if rounded else float
    return dict(b2=r(betas[1]), w1=r(1.0 - betas[0]), w2=r(1.0 - betas[1]), eps=r(eps), mn=r(max_norm), e6=r(1e-6), gs=r(grad_scale))


def reference(p0, g, m0, v0, t, lr, max_norm, clip_n, grad_scale=1.0, betas=BETAS, eps=EPS, rounded=True):
    """dict(norm, coef, gc, m, v, p, S_m, S_p) in float64.  ``gc`` is the gradient the optimizer consumed (scaled, and clipped on
    ``[:clip_n]``); ``S_m`` / ``S_p`` are the scales of ``m`` and ``p`` (the sum of the absolute terms behind each element)."""
    h = _hyper(max_norm, grad_scale, betas, eps, rounded)
    p0, g, m0, v0 = (np.asarray(x, dtype=np.float64) for x in (p0, g, m0, v0))
    lr = f32(lr) if rounded else float(lr)        # the kernels read the learning rate from an fp32 device scalar
    with np.errstate(all="ignore"):
        gs = g * h["gs"]
        norm = math.sqrt(float(np.sum(gs[:clip_n] * gs[:clip_n]))) if clip_n else 0.0
        coef = h["mn"] / (norm + h["e6"])
        if coef >= 1.0:                           # NaN stays NaN, as torch's clamp keeps it
            coef = 1.0
        gc = gs.copy()
        gc[:clip_n] = gc[:clip_n] * coef
        m = m0 + h["w1"] * (gc - m0)              # torch: exp_avg.lerp_(grad, 1 - beta1)
        v = v0 * h["b2"] + h["w2"] * gc * gc
        bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
        step_size = lr / bc1
        denom = np.sqrt(v) / math.sqrt(bc2) + h["eps"]
        p = p0 - step_size * (m / denom)
        S_m = np.abs(m0) + h["w1"] * (np.abs(gc) + np.abs(m0))
        S_p = np.abs(p0) + step_size * S_m / denom
    return dict(norm=norm, coef=coef, gc=gc, m=m, v=v, p=p, S_m=S_m, S_p=S_p)


# ------------------------------------------------------------------------------------------------ metric
def _rel(x, x64, scale):
    """max over elements of |x - x64| / scale; where the scale is 0 the value must be exactly x64 (else inf); a non-finite x is inf."""
    x, x64, scale = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (x, x64, scale))
    if x.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(x - x64)
        r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(x), r, np.inf)
    return float(r.max())


def metrics(got, ref, mask=None, quantities=QUANTITIES):
    """{quantity: metric} of ``got`` (dict with any of norm, gc, m, v, p) against ``reference``'s dict.  ``mask``: the elements to
    judge (the non-finite tests judge the elements fp32 torch leaves finite); None judges every element."""
    out = collections.OrderedDict()
    sel = slice(None) if mask is None else mask
    for q in quantities:
        if q not in got or got[q] is None:
            continue
        x = np.asarray(got[q], dtype=np.float64)
        if q == "norm":
            out[q] = _rel(x, ref["norm"], abs(ref["norm"]))
        else:
            scale = {"gc": np.abs(ref["gc"]), "m": ref["S_m"], "v": ref["v"], "p": ref["S_p"]}[q]
            out[q] = _rel(x.reshape(-1)[sel], ref[q][sel], scale[sel])
    return out


# ------------------------------------------------------------------------------------------------ yardstick
def torch_run(case, device="cpu", dtype=torch.float32, rounded=True):
    """The case through torch's clip + single-tensor Adam in ``dtype`` on ``device``: dict(norm, gc, m, v, p) as numpy arrays."""
    n, k, t = case["n"], case["clip_n"], case["t"]
    r = f32 if rounded else float
    dev = torch.device(device)
    mk = lambda a: torch.from_numpy(np.asarray(a)).to(device=dev, dtype=dtype)      # noqa: E731
    p = torch.nn.Parameter(mk(case["p0"]).clone())
    p.grad = mk(case["g"]) * r(case["grad_scale"])
    if k:
        sl = torch.nn.Parameter(torch.zeros(k, device=dev, dtype=dtype))
        sl.grad = p.grad[:k]                      # a view: the clip scales the leading slice of p.grad in place
        norm = torch.nn.utils.clip_grad_norm_([sl], r(case["max_norm"]), foreach=False)
    else:
        norm = torch.zeros((), device=dev, dtype=dtype)
    opt = torch.optim.Adam([p], lr=r(case["lr"]), betas=case["betas"], eps=case["eps"], foreach=False, fused=False, capturable=False)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=mk(case["m0"]).clone(), exp_avg_sq=mk(case["v0"]).clone())
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t and n == p.numel()
    cpu = lambda x: x.detach().double().cpu().numpy()      # noqa: E731
    return dict(norm=float(norm.double()), gc=cpu(p.grad), m=cpu(st["exp_avg"]), v=cpu(st["exp_avg_sq"]), p=cpu(p))


def reference_of(case, rounded=True):
    return reference(case["p0"], case["g"], case["m0"], case["v0"], case["t"], case["lr"], case["max_norm"], case["clip_n"],
                     case["grad_scale"], case["betas"], case["eps"], rounded)


def yardstick(case, ref, device="cpu", mask=None):
    """(Y per quantity, floored at 2^-24; torch's fp32 outputs)."""
    got = torch_run(case, device)
    return collections.OrderedDict((q, max(x, ULP32)) for q, x in metrics(got, ref, mask).items()), got


def check(label, got, ref, Y, mask=None, quantities=QUANTITIES, margins=MARGINS):
    """The bars of one launch: metric <= margin * Y for every quantity ``got`` holds.  Prints every figure, then asserts.  Returns
    {quantity: (metric, Y, ratio)}."""
    m = metrics(got, ref, mask, quantities)
    out = collections.OrderedDict((q, (x, Y[q], x / Y[q])) for q, x in m.items())
    print(f"\n[{label}] " + ", ".join(f"{q} {x:.3e} = {r:.2f} x Y ({y:.3e}, margin {margins[q]:g})" for q, (x, y, r) in out.items()))
    for q, (x, y, r) in out.items():
        assert x <= margins[q] * y, (label, q, x, y, r)
    return out


def classes(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf per element."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))


# ------------------------------------------------------------------------------------------------ a second correct formulation
MUTANTS = ("no_1e6", "clip_past_clip_n", "t_minus_1", "pow_f32", "eps_inside_bc2", "sqrt_v_plus_eps2", "no_bc2", "m_unclipped",
           "v_unclipped", "grad_scale_twice")


def replay_fp32(case, mutant=None):
    """adam_math.h's operation order in numpy float32: ``(g * gscale) * coef``, ``m0 + w1 * (gi - m0)``, ``v0 * b2 + (w2 * gi) * gi``,
    ``sqrtf(v) / bc2_sqrt + eps``, ``p - step_size * (m / denom)``; the norm's sum in float64 over the fp32 products ``g * gscale``; the
    bias corrections in float64, rounded once.  ``mutant``: one of ``MUTANTS``, a wrong variant the bars must reject."""
    assert mutant is None or mutant in MUTANTS, mutant
    F = np.float32
    k, t, betas = case["clip_n"], case["t"], case["betas"]
    p0, g, m0, v0 = (np.asarray(case[x], dtype=F) for x in ("p0", "g", "m0", "v0"))
    gscale, max_norm = F(case["grad_scale"]), F(case["max_norm"])
    w1, b2, w2, eps = F(1.0 - betas[0]), F(betas[1]), F(1.0 - betas[1]), F(case["eps"])
    with np.errstate(all="ignore"):
        gs = g * gscale
        norm = F(math.sqrt(float(np.sum(gs[:k].astype(np.float64) ** 2)))) if k else F(0.0)
        coef = max_norm / (norm if mutant == "no_1e6" else norm + F(1e-6))
        if coef >= F(1.0):
            coef = F(1.0)
        tt = t - 1 if mutant == "t_minus_1" else t
        if mutant == "pow_f32":
            bc1, bc2 = float(F(1.0) - np.power(F(betas[0]), F(tt))), float(F(1.0) - np.power(F(betas[1]), F(tt)))
        else:
            bc1, bc2 = 1.0 - betas[0] ** tt, 1.0 - betas[1] ** tt
        step_size = F(np.float64(F(case["lr"])) / np.float64(bc1))
        bc2_sqrt = F(np.sqrt(np.float64(bc2)))
        if mutant == "grad_scale_twice":
            gs = gs * gscale
        clipped = np.ones(g.shape, dtype=bool) if mutant == "clip_past_clip_n" else np.arange(g.size) < k
        gi = np.where(clipped, gs * coef, gs).astype(F)
        gm = gs if mutant == "m_unclipped" else gi
        gv = gs if mutant == "v_unclipped" else gi
        m = m0 + w1 * (gm - m0)
        v = v0 * b2 + (w2 * gv) * gv
        if mutant == "eps_inside_bc2":
            denom = (np.sqrt(v) + eps) / bc2_sqrt
        elif mutant == "sqrt_v_plus_eps2":
            denom = np.sqrt(v + eps * eps) / bc2_sqrt
        elif mutant == "no_bc2":
            denom = np.sqrt(v) + eps
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps
        p = p0 - step_size * (m / denom)
    assert all(a.dtype == F for a in (gi, m, v, p))
    return dict(norm=float(norm), gc=gi, m=m, v=v, p=p)


# ------------------------------------------------------------------------------------------------ inputs
def build(n, gscale, state, t, lr, p0_kind, clip_n=None, grad_scale=1.0, seed=0, max_norm=MAX_NORM, betas=BETAS, eps=EPS):
    """A case: dict of fp32 arrays p0, g, m0, v0 and the scalars.  ``gscale``: "inactive" (1e-3: no clip at max_norm 0.5), "active" (10)
    or "edge" (g rescaled so that the clipped slice's norm is 1.5 * max_norm, where the +1e-6 term is worth ~20 ulp of the
    coefficient); about 5 % of g is exactly 0.  ``state``: "zero" or "warm" (m0 ~ 0.3 * s, v0 ~ 0.5 * s^2 for the gradient's scale s,
    5 % of the elements with m0 = v0 = 0, so that denom = eps where g is 0 too).  ``p0_kind``: "random" or "zero"."""
    assert gscale in GSCALES and state in ("zero", "warm") and p0_kind in P0S and (state == "warm" or t == 1)
    clip_n = n if clip_n is None else clip_n
    assert 0 <= clip_n <= n
    rs = np.random.RandomState(seed)
    g = rs.standard_normal(n) * {"inactive": 1e-3, "active": 10.0, "edge": 1.0}[gscale]
    zero = rs.random_sample(n) < 0.05
    if n > 2:
        zero[rs.randint(n)] = True
    g[zero] = 0.0
    if gscale == "edge":
        sl = g[:clip_n] if clip_n else g
        nrm = math.sqrt(float(np.sum((sl * f32(grad_scale)) ** 2)))
        if nrm > 0:
            g = g * (1.5 * max_norm / nrm)
    g = g.astype(np.float32)
    s = float(np.sqrt(np.mean((g.astype(np.float64) * f32(grad_scale)) ** 2))) or 1e-3
    if state == "warm":
        m0 = 0.3 * s * rs.standard_normal(n)
        v0 = 0.5 * s * s * (0.25 + rs.random_sample(n))
        cold = rs.random_sample(n) < 0.05
        if n > 2:
            cold[np.flatnonzero(zero)[0]] = True          # at least one element with g = m0 = v0 = 0
        m0[cold], v0[cold] = 0.0, 0.0
    else:
        m0, v0 = np.zeros(n), np.zeros(n)
    p0 = rs.standard_normal(n) if p0_kind == "random" else np.zeros(n)
    case = dict(n=n, clip_n=clip_n, t=int(t), lr=float(lr), max_norm=f32(max_norm), grad_scale=float(grad_scale), betas=betas, eps=eps,
                p0=p0.astype(np.float32), g=g, m0=m0.astype(np.float32), v0=v0.astype(np.float32),
                id=f"n{n}-clip{clip_n}-{gscale}-{state}-t{t}-lr{lr:g}-p{p0_kind}-gs{grad_scale:.3g}")
    assert_input_condition(case)
    return case


def assert_input_condition(case, ref=None):
    """In fp64: every non-zero g, gc, v0, v and g^2 * (1 - beta2) lies in fp32's normal range, and sum g^2 does not overflow fp32 (the
    yardstick forms it in fp32)."""
    ref = ref or reference_of(case)
    g = np.asarray(case["g"], dtype=np.float64) * f32(case["grad_scale"])
    w2 = f32(1.0 - case["betas"][1])
    for name, x in (("g", np.asarray(case["g"], dtype=np.float64)), ("g * grad_scale", g), ("gc", ref["gc"]), ("v0", np.asarray(case["v0"], dtype=np.float64)),
                    ("v", ref["v"]), ("g^2 (1 - beta2)", g * g * w2), ("gc^2 (1 - beta2)", ref["gc"] ** 2 * w2)):
        a = np.abs(x[x != 0])
        assert a.size == 0 or (a.min() >= F32_TINY and a.max() <= F32_MAX), (case["id"], name, float(a.min()), float(a.max()))
    assert float(np.sum(g * g)) < F32_MAX, case["id"]


def regime_grid():
    """Every (gscale, (state, t), lr, p0) of the regime grid: 3 x 6 x 2 x 2 = 72 combinations."""
    return [(gs, st, lr, p0) for gs in GSCALES for st in STATES for lr in LRS for p0 in P0S]


def case_seed(n, i, salt=0):
    return (n * 7919 + i * 104729 + salt * 15485863) % (2 ** 31 - 1)


def thinned_cases(sizes, clip_ns=("n", "n//3", "1", "0"), big=(17101,), per_big=6, per_small=3):
    """About forty K6b cases over ``sizes``: every value of every regime appears at each size of ``big`` (six cases each: the six
    (state, t) pairs, with gradient scale, lr, p0 and clip_n cycling); ``per_small`` cases at every other size."""
    out, i = [], 0
    for n in sizes:
        for j in range(per_big if n in big else per_small):
            st = STATES[(i if n not in big else j) % len(STATES)]
            gs, lr, p0 = GSCALES[i % 3], LRS[(i // 3 + j) % 2], P0S[(i + j // 2) % 2]
            ck = clip_ns[i % len(clip_ns)]
            clip_n = {"n": n, "n//3": n // 3, "1": min(1, n), "0": 0}[ck]
            out.append(dict(n=n, gscale=gs, state=st[0], t=st[1], lr=lr, p0_kind=p0, clip_n=clip_n, seed=case_seed(n, i)))
            i += 1
    return out


# ------------------------------------------------------------------------------------------------ the GPU tests' synthetic cases
# K6 / K6b: every size at which clip.hip takes another path -- below / at / above one workgroup's 256 threads and its 1024 elements,
# the 2 x 64 bucket of D 64, A 6 (17101), and one workgroup more than kMaxBlocks = 512 (the grid-stride loops take an uneven extra turn)
SIZES = (1, 3, 255, 256, 257, 1023, 1025, 17101, 524288 + 1025)
BIG = (17101, 524288 + 1025)
K6B_CASES = thinned_cases(SIZES, big=BIG)
K6_CASES = ([dict(n=n, gscale=GSCALES[i % 3], state="zero", t=1, lr=3e-4, p0_kind="zero", clip_n=n, seed=case_seed(n, i, 1)) for i, n in enumerate(SIZES)]
            + [dict(n=n, gscale=gs, state="zero", t=1, lr=3e-4, p0_kind="zero", clip_n=n, seed=case_seed(n, 7, 1)) for n in BIG for gs in GSCALES if gs != GSCALES[SIZES.index(n) % 3]])
# mlp_ppo_apply / mlp_ppo_apply_parts: 2 x 64 policies (D, A, continuous)
APPLY_POLICIES = [(64, 6, True), (17, 6, True), (1, 6, True), (64, 4, False), (17, 4, False), (1, 4, False)]


def policy_n_params(D, A, cont, hidden=64, layers=2):
    per = lambda out: sum(a * b + b for a, b in zip([D] + [hidden] * layers, [hidden] * layers + [out]))      # noqa: E731
    return per(A) + per(1) + (A if cont else 0)


def apply_cases(pol):
    """Six cases per policy; over the six policies every (grad_scale, clip regime, t in {1, 1000}) combination appears twice."""
    pi = APPLY_POLICIES.index(pol)
    out = []
    for j in range(6):
        k = pi * 6 + j
        t = (1, 1000)[(k // 9) % 2]
        out.append(dict(gscale=GSCALES[(k // 3) % 3], state="zero" if t == 1 and j % 2 else "warm", t=t, lr=LRS[j % 2], p0_kind=P0S[(j // 2) % 2],
                        grad_scale=GRAD_SCALES[k % 3], seed=case_seed(pi, j, 2)))
    return out


def parts_cases(pol):
    """(case, partition) per policy: the clip's partial sums as n_part in {1, 255, 257, aurppo_p2p_parts(n)} sums, and once as
    aurppo_p2p_parts(n) entries of which all but three are 0."""
    pi = APPLY_POLICIES.index(pol)
    out = []
    for j, parts in enumerate((1, 255, 257, "p2p", "p2p-sparse")):
        k = pi * 5 + j
        t = (1, 1000)[k % 2]
        out.append((dict(gscale=GSCALES[k % 3], state="zero" if t == 1 and k % 4 == 1 else "warm", t=t, lr=LRS[(k // 2) % 2], p0_kind=P0S[(k // 3) % 2],
                         grad_scale=1.0, seed=case_seed(pi, j, 3)), parts))
    return out


def host_sq_parts(g, n_part, sparse=False):
    """Partial sums of squares of ``g`` in fp64, as ``n_part`` entries: contiguous chunks, or (``sparse``) three chunks in the first,
    middle and last entry and zeros elsewhere."""
    g = np.asarray(g, dtype=np.float64)
    if sparse:
        out = np.zeros(n_part)
        for at, ch in zip(sorted({0, n_part // 2, n_part - 1}), np.array_split(g, len({0, n_part // 2, n_part - 1}))):
            out[at] = np.sum(ch * ch)
        return out
    return np.array([np.sum(ch * ch) for ch in np.array_split(g, n_part)])


# ------------------------------------------------------------------------------------------------ launching the kernels (GPU)
def _dev(case, t_before):
    mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    lr = torch.tensor([case["lr"]], dtype=torch.float32, device="cuda")
    step = torch.tensor([float(t_before)], dtype=torch.float32, device="cuda")
    return mk(case["p0"]), mk(case["g"]), mk(case["m0"]), mk(case["v0"]), lr, step, torch.full((1,), float("nan"), device="cuda")


def outputs(norm, g, m, v, p, n):
    """The first ``n`` elements of a launch's device buffers as the dict ``metrics`` takes."""
    torch.cuda.synchronize()
    cpu = lambda x: x[:n].detach().cpu().numpy().copy()      # noqa: E731
    return dict(norm=float(norm[0]), gc=None if g is None else cpu(g), m=cpu(m), v=cpu(v), p=cpu(p))


def run_k6(case):
    """``hip_ops.grad_norm_clip_`` (k_sqnorm, k_clip_scale): dict(norm, gc)."""
    from aur_ppo_amd import hip_ops as H
    assert case["grad_scale"] == 1.0 and case["clip_n"] == case["n"]
    g = torch.from_numpy(case["g"].copy()).cuda()
    norm = H.grad_norm_clip_(g, case["max_norm"])
    torch.cuda.synchronize()
    return dict(norm=float(norm[0]), gc=g.cpu().numpy())


def run_k6b(case):
    """``hip_ops.clip_adam_`` (k_sqnorm_step, k_clip_adam); the kernel advances the step count itself.  (outputs, step count after)."""
    from aur_ppo_amd import hip_ops as H
    assert case["grad_scale"] == 1.0
    p, g, m, v, lr, step, norm = _dev(case, case["t"] - 1)
    H.clip_adam_(p, g, m, v, lr, step, case["max_norm"], case["clip_n"], case["betas"], case["eps"], norm)
    return outputs(norm, g, m, v, p, case["n"]), float(step)


def run_apply(case, lay, parts=None, misalign=False):
    """``hip_ops.mlp_ppo_apply`` (k_adam_chain forms the norm of g * grad_scale itself and leaves g alone) or, with ``parts`` (a host
    fp64 array), ``mlp_ppo_apply_parts`` (the norm is the sum of the parts; the clipped gradient is stored).  The step count is the
    caller's (``mlp_ppo_grad`` advances it).  ``misalign``: the gradient is a view that starts 4 bytes into its buffer.
    Returns (outputs, step count after, the gradient buffer after as int32 bits)."""
    from aur_ppo_amd import hip_ops as H
    assert case["clip_n"] == case["n"] == lay["n_params"]
    p, g, m, v, lr, step, norm = _dev(case, case["t"])
    if misalign:
        buf = torch.zeros(case["n"] + 1, device="cuda")
        buf[1:] = g
        g = buf[1:]
        assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    if parts is None:
        H.mlp_ppo_apply(p, g, m, v, lay, lr, step, case["max_norm"], case["betas"], case["eps"], norm, grad_scale=case["grad_scale"])
    else:
        assert case["grad_scale"] == 1.0
        H.mlp_ppo_apply_parts(p, g, m, v, lay, lr, step, case["max_norm"], case["betas"], case["eps"], norm,
                              torch.from_numpy(np.ascontiguousarray(parts, dtype=np.float64)).cuda())
    out = outputs(norm, g if parts is not None else None, m, v, p, case["n"])
    return out, float(step), g.view(torch.int32).cpu().numpy()
