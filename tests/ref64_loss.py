"""fp64 reference of the per-op loss path (K4 + K5: csrc/loss.hip through ``hip_ops.loss_fwd_bwd`` / ``loss_fwd_bwd_packed``), the inputs
the fp64 tests feed it, the metric it is judged on, and a numpy-float32 replay of the kernels' arithmetic.  A plain helper module (no
tests in it); DESIGN 2.3 derives the bars, tests/test_loss_fp64_host.py re-derives them on the CPU.

What is here
  * ``run_terms``: ``ref64.loss_terms`` on leaves ``logp, ent, v`` + autograd, in the dtype asked for.  In float64 it is the REFERENCE;
    in float32 (CPU) it is the YARDSTICK Y: what plain fp32 torch loses against fp64 on the same case and metric.
  * ``grad_scales`` / ``array_metrics``: per-sample gradient error over the absolute term behind the element
    (g_newlogp: |an ratio| / M, g_newv: |vf_coef du or dc| / M, g_entropy: ent_coef / M); the nine scalars use ``ref64.scalar_metrics``.
  * ``build_inputs``: the seven input arrays of a case in one of six regimes, moved by ``ref64.make_records_safe`` until NO sample is
    within ``BRANCH_EPS`` of a decision for either normalisation and any value mode (asserted): no test excludes a sample.
  * ``replay``: ppo_sample<true> / adv_mean_std / the fold of loss.hip in numpy float32 (sums in fp64, the final casts), expf evaluated as
    fp64 exp rounded to fp32, optionally with every result moved by one ulp (the device's expf bound); and its WRONG variants.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from tests.ref64 import (BRANCH_EPS, MARGIN_SCALARS, SCALAR_NAMES, TINY_M, ULP32, branch_distances, f32, loss_terms,  # noqa: F401
                         make_records_safe, scalar_metrics)

ARRAYS = ("g_newlogp", "g_newv", "g_entropy")
# Bars: metric <= margin * Y.  tests/test_loss_fp64_host.py derives every figure from ``replay`` (never from a kernel): the smallest
# power of two that covers twice the worst draw.  At M >= TINY_M the scalars fit ref64.MARGIN_SCALARS, which is reused; below it they do not.
MARGINS = {"g_newlogp": 8.0, "g_newv": 2.0, "g_entropy": 4.0}                 # M >= TINY_M
MARGINS_TINY_M = {"g_newlogp": 8.0, "g_newv": 2.0, "g_entropy": 4.0}          # M < TINY_M: Y is the rounding of a handful of samples
MARGIN_SCALARS_TINY_M = 32.0                                                  # the nine scalars at M < TINY_M

HYPERS = (dict(clip=0.2, ent_coef=0.01, vf_coef=0.5), dict(clip=0.1, ent_coef=0.0, vf_coef=1.0), dict(clip=0.3, ent_coef=0.05, vf_coef=0.25))
REGIMES = ("normal", "offset", "tiny", "wide", "vclip", "const")
COMBOS = tuple((na, vm) for na in (0, 1) for vm in (0, 1, 2))         # (norm_adv, value mode): all six
INPUTS = ("newlogp", "newv", "entropy", "rec")                          # rec: (M, 4) = {old_logp, adv, ret, old_v}
F = np.float32


def margin(name, M):
    return (MARGINS if M >= TINY_M else MARGINS_TINY_M)[name]


def scalar_margin(M):
    return MARGIN_SCALARS if M >= TINY_M else MARGIN_SCALARS_TINY_M


# ------------------------------------------------------------------------------------------------ inputs
def case_seed(M, regime, hyper_i, draw=0):
    return (M * 31 + REGIMES.index(regime) * 7919 + hyper_i * 104729 + draw * 15485863) % (2 ** 31 - 1)


def build_inputs(M, regime="normal", hyper_i=0, draw=0):
    """CPU fp32 tensors ``newlogp, newv, entropy`` (M,) and ``rec`` (M, 4).  ``normal`` is the distribution of
    test_hip_parity.py::test_loss_vs_c_oracle; the other regimes change one thing each:
      offset  advantage mean 100 x its std (none within 0.35 std of the mean: no sample's scale drowns in the mean's rounding);  tiny  advantages x 1e-4;  const  every advantage 0.75 (normalised: exactly 0);
      wide    log-ratio spread so that about a third of the samples clip on each side;  vclip  about half of |v - v_old| beyond clip.
    Asserts that zero samples lie within BRANCH_EPS of a branch for norm_adv in {0, 1} and every value mode."""
    assert regime in REGIMES
    clip = HYPERS[hyper_i]["clip"]
    rs = np.random.RandomState(case_seed(M, regime, hyper_i, draw))
    oldlp = -1 + 0.5 * rs.standard_normal(M)
    newlp = oldlp + (clip / 0.43 if regime == "wide" else 0.2) * rs.standard_normal(M)
    adv0 = 3 * rs.standard_normal(M) + 0.5
    oldv = rs.standard_normal(M)
    newv = oldv + (clip / 0.674 if regime == "vclip" else 0.3) * rs.standard_normal(M)
    ret = oldv + adv0
    ent = rs.random_sample(M) + 1
    adv = {"normal": adv0, "wide": adv0, "vclip": adv0, "offset": 300.0 + 2.097 * np.sign(adv0 - 0.5) * (0.5 + np.abs(adv0 - 0.5) / 3), "tiny": adv0 * 1e-4,
           "const": np.full(M, 0.75)}[regime]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))          # noqa: E731
    x = dict(newlogp=t(newlp), newv=t(newv), entropy=t(ent), rec=torch.stack([t(oldlp), t(adv), t(ret), t(oldv)], 1).contiguous())
    x["moved"] = make_safe(x, clip)
    return x


def make_safe(x, clip):
    """``make_records_safe`` for both normalisations in value mode 1 (whose decisions include those of modes 0 and 2; the advantages
    never move, so the normalised advantage is fixed), repeated until neither moves a record.  Returns how many records moved."""
    M = x["newlogp"].numel()
    lp, v, idx = x["newlogp"].double(), x["newv"].double(), torch.arange(M)
    moved = 0
    for _ in range(8):
        n = sum(make_records_safe(lp, v, x["rec"], idx, clip, bool(na) and M > 1, 1) for na in (1, 0))
        moved += n
        if n == 0:
            break
    assert_safe(x, clip)
    return moved


def assert_safe(x, clip):
    """ZERO samples within BRANCH_EPS of a decision, for every (norm_adv, value mode)."""
    M = x["newlogp"].numel()
    for na, vm in COMBOS:
        if na and M == 1:
            continue                    # std of one sample is NaN: every output that depends on it is NaN, there is no decision
        d = branch_distances(x["newlogp"].double(), x["newv"].double(), x["rec"], clip, bool(na), vm)
        n_unsafe = int(sum((t < BRANCH_EPS).sum() for t in d.values() if torch.is_tensor(t)))
        assert n_unsafe == 0, (na, vm, n_unsafe)


# ------------------------------------------------------------------------------------------------ reference, yardstick
def run_terms(x, hyper, norm_adv, vmode, dtype=torch.float64):
    """``loss_terms`` + autograd in ``dtype`` on the CPU: scalars (9), their scales, and the three per-sample gradients."""
    logp, ent, v = (x[k].detach().to(dtype).clone().requires_grad_() for k in ("newlogp", "entropy", "newv"))
    loss, sc, ssc = loss_terms(logp, ent, v, x["rec"].to(dtype), hyper["clip"], hyper["ent_coef"], hyper["vf_coef"], bool(norm_adv), vmode)
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad          # noqa: E731
    return dict(scalars=sc, scalar_scales=ssc, g_newlogp=zero(logp), g_newv=zero(v), g_entropy=zero(ent))


def grad_scales(x, hyper, norm_adv, vmode):
    """fp64, per sample: the absolute term behind each gradient element (the term the active branch differentiates)."""
    c, ec, vc = f32(hyper["clip"]), f32(hyper["ent_coef"]), f32(hyper["vf_coef"])
    rec = x["rec"].double()
    old_lp, adv, ret, old_v = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    lp, v = x["newlogp"].double(), x["newv"].double()
    M = lp.numel()
    ratio = (lp - old_lp).exp()
    std = adv.std() if M > 1 else torch.full((), float("nan"), dtype=torch.float64)
    an = (adv - adv.mean()) / (std + 1e-8) if norm_adv else adv
    du = v - (old_v if vmode == 2 else ret)
    if vmode == 1:
        dc = old_v + (v - old_v).clamp(-c, c) - ret
        du = torch.where(du * du > dc * dc, du, dc)
    return dict(g_newlogp=(an * ratio).abs() / M, g_newv=(vc * du).abs() / M, g_entropy=torch.full_like(lp, ec / M))


def reference(x, hyper, norm_adv, vmode):
    ref = run_terms(x, hyper, norm_adv, vmode, torch.float64)
    ref["scales"] = grad_scales(x, hyper, norm_adv, vmode)
    return ref


def array_metrics(got, ref, only=None):
    """{array: max over samples of |g - g64| / S}.  Where the reference is NaN (M = 1 with normalisation) the array must be NaN; everywhere
    else it must be finite; where S is 0 (normalised constant advantages, ent_coef = 0) it must EQUAL the reference.  ``only``: a
    boolean mask of the samples to judge (the non-finite tests judge the untouched samples)."""
    out = collections.OrderedDict()
    for n in ARRAYS:
        g = torch.as_tensor(got[n]).detach().double().cpu().reshape(-1)
        g64, S = ref[n].reshape(-1), ref["scales"][n]
        if only is not None:
            g, g64, S = g[only], g64[only], S[only]
        nan = torch.isnan(g64) | torch.isnan(S)
        assert bool(torch.isnan(g[nan]).all()), f"{n}: expected NaN where the reference is NaN"
        g, g64, S = g[~nan], g64[~nan], S[~nan]
        assert bool(torch.isfinite(g).all()), f"{n}: non-finite gradient"
        err = (g - g64).abs()
        m = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        out[n] = float(m.max()) if m.numel() else 0.0
    return out


def yardstick(x, hyper, norm_adv, vmode, ref):
    """Plain fp32 torch autograd on the CPU against fp64 on the same metrics, floored at one fp32 ulp of the scale.
    Returns ({array: Y}, Y of the scalars = the worst of the nine)."""
    got = run_terms(x, hyper, norm_adv, vmode, torch.float32)
    Ya = {n: max(m, ULP32) for n, m in array_metrics(got, ref).items()}
    Ys = max(max(m, ULP32) for m in scalar_metrics(got["scalars"], ref).values())
    return Ya, Ys


def ratios(got, ref, Y, only=None):
    """(per-array metric, per-scalar metric, {class: metric / Y}) of one result; asserts the NaN / finiteness rules on the way."""
    Ya, Ys = Y
    am = array_metrics(got, ref, only)
    sm = scalar_metrics(got["scalars"], ref) if only is None else {}
    r = collections.OrderedDict((n, am[n] / Ya[n]) for n in ARRAYS)
    if sm:
        r["scalars"] = max(sm.values()) / Ys
    return am, sm, r


def check(got, ref, Y, M, label="", only=None):
    """The bars of one result: every array <= margin(array, M) * Y, every scalar <= scalar_margin(M) * Y.  Prints, then asserts."""
    am, sm, r = ratios(got, ref, Y, only)
    print(f"\n[{label}] " + "  ".join(f"{n} {am[n]:.3e} = {r[n]:.2f} x Y ({Y[0][n]:.3e}, margin {margin(n, M):g})" for n in ARRAYS)
          + (f"  scalars {max(sm, key=sm.get)} {max(sm.values()):.3e} = {r['scalars']:.2f} x Y ({Y[1]:.3e}, margin {MARGIN_SCALARS:g})" if sm else ""))
    for n in ARRAYS:
        assert am[n] <= margin(n, M) * Y[0][n], (label, n, am[n], Y[0][n], r[n])
    for n, m in sm.items():
        assert m <= scalar_margin(M) * Y[1], (label, n, m, Y[1], m / Y[1])
    return r


# ------------------------------------------------------------------------------------------------ numpy-float32 replay
# variant -> what it gets wrong.  tests/test_loss_fp64_host.py names beside each the regime in which the bars must reject it.
VARIANTS = collections.OrderedDict([
    ("std_over_M", "variance over M instead of M - 1"),
    ("stats_fp32", "advantage sum and sum of squares each accumulated in one running fp32 sum"),
    ("vl_no_half", "vl without its 0.5"),
    ("g_newv_no_vf_coef", "g_newv without vf_coef"),
    ("g_entropy_no_invM", "g_entropy without 1 / M"),
    ("g_entropy_wrong_sign", "g_entropy = +ent_coef / M"),
    ("kl_swapped", "kl and old_kl swapped"),
    ("vmode_0_2_swapped", "value modes 0 and 2 swapped"),
    ("packed_ret_oldv_swapped", "packed record fields ret and old_v swapped"),
    ("last_block_dropped", "the last partial 1024-sample block left out of every sum"),
    ("stash_missing", "the mean / std stash not reaching adv_mean / adv_std (they read 0)"),
    ("loss_no_entropy", "loss formed without the entropy term"),
])


def _expf(lr, perturb):
    """fp64 exp rounded to fp32; ``perturb``: every finite result moved one ulp, up on even samples and down on odd ones."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.exp(lr.astype(np.float64)).astype(F)
    if perturb:
        up = (np.arange(r.size) % 2) == 0
        r = np.where(up, np.nextafter(r, F(np.inf)), np.nextafter(r, F(0))).astype(F)
    return r


def _gate(t, inside):
    """ppo_gate<true>: t where the clamp passes gradient, a zero of t's sign elsewhere (t * 0 for a finite t)."""
    return np.where(inside != 0, t, np.copysign(F(0), t)).astype(F)


def replay(x, hyper, norm_adv, vmode, perturb=False, variant=None):
    """loss.hip in numpy float32, operation for operation (ppo_math.h's ppo_sample and adv_mean_std, k_loss_final's fold).  The
    library is built without fma contraction and with correctly rounded division and square root, so every operation but expf rounds as here."""
    assert variant is None or variant in VARIANTS, variant
    nl, nv, en = (x[k].numpy().astype(F).reshape(-1) for k in ("newlogp", "newv", "entropy"))
    rec = x["rec"].numpy().astype(F)
    ol, adv, R, vo = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    if variant == "packed_ret_oldv_swapped":
        R, vo = vo, R
    if variant == "vmode_0_2_swapped":
        vmode = {0: 2, 1: 1, 2: 0}[vmode]
    M = nl.size
    keep = (M // 1024) * 1024 if variant == "last_block_dropped" else M
    clip, lo, hi = F(hyper["clip"]), F(1.0 - hyper["clip"]), F(1.0 + hyper["clip"])
    ec, vc = F(hyper["ent_coef"]), F(hyper["vf_coef"])
    with np.errstate(all="ignore"):
        # ---- k_adv_stats + adv_mean_std
        if variant == "stats_fp32":
            ts, tq = (np.cumsum(a, dtype=F)[-1] if a.size else F(0) for a in (adv[:keep], adv[:keep] * adv[:keep]))       # one running fp32 sum each
            m = ts / F(M)
            var = (tq - ts * m) / F(M - 1)
            mean, std = F(m), F(np.sqrt(max(var, F(0)))) if not np.isnan(var) else F(np.nan)
        else:
            a64 = adv[:keep].astype(np.float64)
            ts, tq = np.float64(a64.sum()), np.float64((a64 * a64).sum())
            m = ts / np.float64(M)
            var = (tq - ts * m) / np.float64(M if variant == "std_over_M" else M - 1)
            if var < 0.0:
                var = np.float64(0.0)
            mean, std = F(m), F(np.sqrt(var))
        denom = F(std + F(1e-8))
        invM = F(1.0) / F(M)
        # ---- ppo_sample
        lr = nl - ol
        ratio = _expf(lr, perturb)
        an = ((adv - mean) / denom).astype(F) if norm_adv else adv
        okl = -lr
        kl = (ratio - F(1)) - lr
        cf = (np.abs(ratio - F(1)) > clip).astype(F)
        rc = np.minimum(np.maximum(ratio, lo), hi)                        # ppo_clamp<true>: NaN stays NaN
        l1, l2 = -an * ratio, -an * rc
        pg = np.maximum(l1, l2)                                            # ppo_max<true>
        w1 = np.where(l1 > l2, F(1), np.where(l1 == l2, F(0.5), F(0))).astype(F)
        inr = ((ratio >= lo) & (ratio <= hi)).astype(F)
        dpg = (w1 * (-an) + _gate((F(1) - w1) * (-an), inr)) * invM
        g_lp = dpg * ratio
        if vmode == 1:
            du = nv - R
            vu = du * du
            dv = nv - vo
            dcl = np.minimum(np.maximum(dv, -clip), clip)
            dc = (vo + dcl) - R
            vcl = dc * dc
            vl = np.maximum(vu, vcl)
            u1 = np.where(vu > vcl, F(1), np.where(vu == vcl, F(0.5), F(0))).astype(F)
            inv = ((dv >= -clip) & (dv <= clip)).astype(F)
            dvl = (u1 * (F(2) * du) + _gate((F(1) - u1) * (F(2) * dc), inv)) * (F(0.5) * invM)
        else:
            du = nv - (R if vmode == 0 else vo)
            vl = du * du
            dvl = (F(2) * du) * (F(0.5) * invM)
        g_v = dvl if variant == "g_newv_no_vf_coef" else dvl * vc
        g_e = -ec * invM
        if variant == "g_entropy_no_invM":
            g_e = -ec
        if variant == "g_entropy_wrong_sign":
            g_e = ec * invM
        # ---- the six fp64 sums and k_loss_final
        s = lambda a: np.float64(a[:keep].astype(np.float64).sum()) / np.float64(M)          # noqa: E731
        pg_s, vl_s, ent_s = F(s(pg)), F(0.5) * F(s(vl)), F(s(en))
        if variant == "vl_no_half":
            vl_s = F(s(vl))
        okl_s, kl_s, cf_s = F(s(okl)), F(s(kl)), F(s(cf))
        if variant == "kl_swapped":
            okl_s, kl_s = kl_s, okl_s
        loss = (pg_s - ec * ent_s) + vl_s * vc
        if variant == "loss_no_entropy":
            loss = pg_s + vl_s * vc
        m_out, s_out = (F(0), F(0)) if variant == "stash_missing" else (mean, std)
    sc = np.array([loss, pg_s, vl_s, ent_s, okl_s, kl_s, cf_s, m_out, s_out], dtype=F)
    return dict(scalars=torch.from_numpy(sc), g_newlogp=torch.from_numpy(np.ascontiguousarray(g_lp, dtype=F)),
                g_newv=torch.from_numpy(np.ascontiguousarray(g_v, dtype=F)), g_entropy=torch.from_numpy(np.full(M, g_e, dtype=F)))


# ------------------------------------------------------------------------------------------------ launching the kernels (GPU)
def kernel_run(x_gpu, hyper, norm_adv, vmode, packed, out_scalars=None):
    """One call of the per-op loss on GPU tensors ``x_gpu`` (the dict of ``build_inputs`` moved to the device); the packed entry point reads
    the record as it is, the unpacked one its four columns as separate contiguous arrays."""
    from aur_ppo_amd import hip_ops as H
    nl, nv, en, rec = (x_gpu[k] for k in INPUTS)
    if packed:
        out = H.loss_fwd_bwd_packed(nl, nv, en, rec, hyper["clip"], hyper["ent_coef"], hyper["vf_coef"], bool(norm_adv), vmode, out_scalars)
    else:
        cols = x_gpu.get("cols")
        if cols is None:
            cols = x_gpu["cols"] = [rec[:, k].contiguous() for k in range(4)]
        ol, adv, ret, ov = cols
        out = H.loss_fwd_bwd(nl, ol, adv, nv, ov, ret, en, hyper["clip"], hyper["ent_coef"], hyper["vf_coef"], bool(norm_adv), vmode, out_scalars)
    return dict(zip(("scalars",) + ARRAYS, out))
