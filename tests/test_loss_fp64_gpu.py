"""GPU: the per-op loss path (K4 + K5: k_adv_stats<1|4>, k_loss<packed|unpacked>, k_loss_final through ``hip_ops.loss_fwd_bwd`` /
``loss_fwd_bwd_packed``, and the autograd wrappers over them) held to the fp64 reference of tests/ref64_loss.py.  Every bar is either
bit-equality or margin x Y with the margins tests/test_loss_fp64_host.py derives on the CPU; run with ``-s`` for the figures."""
import numpy as np
import pytest
import torch

from tests import ref64_loss as R

pytestmark = pytest.mark.gpu

# 1 ... 257: below a wave, a wave, a workgroup and one sample either side; 1023 ... 1025: one workgroup becomes two; 262145: more than 256
# statistic partials (the strided fold in k_loss); 1047551 ... 1047553: the grid cap of 1023 workgroups and the grid-stride loop's second
# trip; 2095109: a third trip, ragged
SWEEP_M = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 262145, 1047551, 1047552, 1047553, 2095109)
REGIME_M = (65, 1025, 262145)
NAMES = ("scalars",) + R.ARRAYS


@pytest.fixture(scope="module")
def H():
    from aur_ppo_amd import hip_ops
    assert torch.cuda.is_available()
    return hip_ops


_CASES = {}


def _case(M, regime="normal", hi=0):
    """Inputs (CPU and GPU) of a case with the fp64 reference and the yardstick of each (norm_adv, value mode), computed once and left
    unchanged; only the last large case is kept."""
    key = (M, regime, hi)
    if key not in _CASES:
        for k in [k for k in _CASES if k[0] > 4096]:
            del _CASES[k]
        x = R.build_inputs(M, regime, hi)
        _CASES[key] = dict(x=x, gpu={k: x[k].cuda() for k in R.INPUTS}, ref={})
    return _CASES[key]


def _ref(case, hi, na, vm):
    if (na, vm) not in case["ref"]:
        ref = R.reference(case["x"], R.HYPERS[hi], na, vm)
        case["ref"][(na, vm)] = (ref, R.yardstick(case["x"], R.HYPERS[hi], na, vm, ref))
    return case["ref"][(na, vm)]


def _bits_equal(a, b):
    return all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in NAMES)


def _both_entry_points(case, hi, na, vm, label):
    """Both entry points on one case: each within the bars, and bit-equal to each other."""
    M = case["x"]["newlogp"].numel()
    ref, Y = _ref(case, hi, na, vm)
    got = {packed: R.kernel_run(case["gpu"], R.HYPERS[hi], na, vm, packed) for packed in (False, True)}
    for packed, g in got.items():
        R.check(g, ref, Y, M, f"{label}-{'packed' if packed else 'unpacked'}")
    assert _bits_equal(got[False], got[True]), f"{label}: packed and unpacked results differ in bits"
    return got[False]


@pytest.mark.parametrize("na,vm", R.COMBOS)
@pytest.mark.parametrize("M", SWEEP_M)
def test_loss_sweep_of_M_within_margin_of_fp64(H, M, na, vm):
    """``normal`` inputs, the default hyperparameters, all six (norm_adv, value mode), both entry points: the three gradient arrays and the
    nine scalars within margin x Y of fp64; at M = 1 with norm_adv NaN exactly where the reference has NaN; packed == unpacked in bits."""
    got = _both_entry_points(_case(M), 0, na, vm, f"M{M}-{'norm' if na else 'raw'}-v{vm}")
    if M == 1 and na:
        ref, _ = _ref(_case(M), 0, na, vm)
        assert bool(torch.isnan(ref["g_newlogp"]).all()) and bool(torch.isnan(got["g_newlogp"]).all())
        assert torch.equal(torch.isnan(got["scalars"]).cpu(), torch.isnan(ref["scalars"]))


@pytest.mark.parametrize("M", REGIME_M)
@pytest.mark.parametrize("hi", range(len(R.HYPERS)))
@pytest.mark.parametrize("regime", R.REGIMES)
def test_loss_regimes_and_hyperparameters_within_margin_of_fp64(H, regime, hi, M):
    """Every input regime x every hyperparameter set, all six (norm_adv, value mode), both entry points."""
    case = _case(M, regime, hi)
    for na, vm in R.COMBOS:
        got = _both_entry_points(case, hi, na, vm, f"M{M}-{regime}-h{hi}-{'norm' if na else 'raw'}-v{vm}")
        if regime == "const" and na:
            assert bool((got["g_newlogp"] == 0).all()) and float(got["scalars"][H.S_PG]) == 0.0        # normalised advantage exactly 0


# ------------------------------------------------------------------------------------------------ exact branches
def _exact_inputs(kind, M):
    """Hand-built fp32 inputs whose decisions do not depend on expf's rounding.  The log-ratio is 0 (ratio exactly 1) except in ``an_zero``,
    where both surrogates are 0 whatever the ratio and the log-ratios lie far from every edge."""
    i = np.arange(M)
    clip = np.float32(0.2)
    oldlp = (-1.0 - 0.03125 * i).astype(np.float32)
    newlp = oldlp.copy()
    adv = (0.5 * ((i % 7) - 3) + 0.25).astype(np.float32)                                      # +-, none zero
    oldv = (0.125 * ((i % 5) - 2)).astype(np.float32)
    newv = (oldv + np.array([0.0625, -0.125, 0.375, -0.5], np.float32)[i % 4]).astype(np.float32)        # inside and outside the clip
    ret = (oldv + 1.0 + 0.25 * (i % 3)).astype(np.float32)                                     # (v - ret)^2 != (v_clipped - ret)^2
    ent = (1.0 + 0.015625 * i).astype(np.float32)
    if kind == "dv_eq_clip":                    # v - v_old == +-clip exactly: closed-interval clamp gradient, and vu == vc ties
        oldv[:] = 0
        newv = np.where(i % 2 == 0, clip, -clip).astype(np.float32)
    elif kind == "v_eq_ret":
        ret = newv.copy()
    elif kind == "an_zero":
        adv[:] = 0
        newlp = (oldlp + np.array([0.05, -0.05, 0.5, -0.5], np.float32)[i % 4]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))          # noqa: E731
    return dict(newlogp=t(newlp), newv=t(newv), entropy=t(ent), rec=torch.stack([t(oldlp), t(adv), t(ret), t(oldv)], 1).contiguous())


@pytest.mark.parametrize("M", [8, 64])
@pytest.mark.parametrize("kind", ["lr_zero", "dv_eq_clip", "v_eq_ret", "an_zero", "ent_coef_zero"])
def test_loss_exact_branch_conventions_match_torch_autograd(H, kind, M):
    """ppo_math.h's conventions on inputs that sit ON a decision: lr = 0 (ratio exactly 1); v - v_old == +-clip with v_old = 0 and
    v = float32(clip) (the clamp passes gradient on the closed interval, and vu == vc ties split 0.5 / 0.5); v == ret; an == 0 (both
    surrogates tie at 0); ent_coef = 0 (g_entropy exactly +-0).  Per sample against fp32 torch autograd on the CPU at rtol 1e-6, NaN masks
    equal.  ``ratio == lo`` exactly cannot be built without expf (lo is not the exponential of a float), so it is not here."""
    x = _exact_inputs(kind, M)
    hyper = dict(R.HYPERS[0], ent_coef=0.0) if kind == "ent_coef_zero" else R.HYPERS[0]
    gpu = {k: x[k].cuda() for k in R.INPUTS}
    for na, vm in R.COMBOS:
        if kind == "an_zero" and na:
            continue                                    # constant advantages normalise to 0 / 1e-8: the ``const`` regime covers it
        want = R.run_terms(x, hyper, na, vm, torch.float32)
        got = {p: R.kernel_run(gpu, hyper, na, vm, p) for p in (False, True)}
        assert _bits_equal(got[False], got[True])
        for n in R.ARRAYS:
            torch.testing.assert_close(got[False][n].cpu(), want[n], rtol=1e-6, atol=0.0, equal_nan=True, msg=lambda m: f"{kind} {na} {vm} {n}: {m}")
        sc = got[False]["scalars"].cpu()
        assert torch.equal(torch.isnan(sc), torch.isnan(want["scalars"]))
        if kind != "an_zero":
            assert float(sc[H.S_KL]) == 0.0 and float(sc[H.S_OLD_KL]) == 0.0 and float(sc[H.S_CLIPFRAC]) == 0.0
        if kind == "an_zero":
            assert float(sc[H.S_PG]) == 0.0 and bool((got[False]["g_newlogp"] == 0).all())
        if kind == "v_eq_ret" and vm == 0:
            assert float(sc[H.S_VL]) == 0.0 and bool((got[False]["g_newv"] == 0).all())
        if kind == "ent_coef_zero":
            g_e = got[False]["g_entropy"]
            assert bool(torch.isfinite(g_e).all()) and bool((g_e == 0).all())


# ------------------------------------------------------------------------------------------------ non-finite inputs
NONFINITE = ("nan_newlogp", "inf_ratio", "nan_newv", "pinf_ret", "ninf_ret", "nan_adv", "nan_entropy")


def _inject(x, kind, pos):
    """One non-finite VALUE in a float array (every index and size stays valid)."""
    x = {k: x[k].clone() for k in R.INPUTS}
    nan, inf = float("nan"), float("inf")
    if kind == "nan_newlogp":
        x["newlogp"][pos] = nan
    elif kind == "inf_ratio":
        x["newlogp"][pos] = x["rec"][pos, 0] + 200.0            # exp(200) = inf in fp32
    elif kind == "nan_newv":
        x["newv"][pos] = nan
    elif kind in ("pinf_ret", "ninf_ret"):
        x["rec"][pos, 2] = inf if kind == "pinf_ret" else -inf
    elif kind == "nan_adv":
        x["rec"][pos, 1] = nan
    elif kind == "nan_entropy":
        x["entropy"][pos] = nan
    return x


def _pattern(sc):
    sc = sc.detach().cpu().double()
    return "".join("N" if bool(torch.isnan(v)) else ("+" if float(v) == float("inf") else ("-" if float(v) == float("-inf") else ".")) for v in sc)


@pytest.mark.parametrize("pos", [0, 130, 299])
@pytest.mark.parametrize("kind", NONFINITE)
def test_loss_propagates_non_finite_inputs_as_torch_does(H, kind, pos):
    """M = 300, one non-finite value at position 0, inside the third wave, or in the last sample; every other sample finite and
    branch-safe.  Against fp32 torch on the CPU: the NaN / +inf / -inf pattern of the nine scalars equal, the NaN mask of each gradient array
    equal; the gradients of the untouched samples within margin x Y of fp64 wherever the reference's are finite."""
    M = 300
    x = _inject(_case(M)["x"], kind, pos)
    gpu = {k: x[k].cuda() for k in R.INPUTS}
    untouched = torch.ones(M, dtype=torch.bool)
    untouched[pos] = False
    for na, vm in R.COMBOS:
        want = R.run_terms(x, R.HYPERS[0], na, vm, torch.float32)
        ref = R.reference(x, R.HYPERS[0], na, vm)
        got = {p: R.kernel_run(gpu, R.HYPERS[0], na, vm, p) for p in (False, True)}
        for p, g in got.items():
            label = f"{kind}@{pos}-{'norm' if na else 'raw'}-v{vm}-{'packed' if p else 'unpacked'}"
            assert _pattern(g["scalars"]) == _pattern(want["scalars"]), (label, _pattern(g["scalars"]), _pattern(want["scalars"]))
            for n in R.ARRAYS:
                assert torch.equal(torch.isnan(g[n]).cpu(), torch.isnan(want[n])), (label, n)
            only = untouched & torch.stack([torch.isfinite(ref[n]) for n in R.ARRAYS]).all(0) & torch.isfinite(ref["scales"]["g_newlogp"])
            if bool(only.any()):
                Ya = {n: max(m, R.ULP32) for n, m in R.array_metrics(want, ref, only).items()}
                R.check(g, ref, (Ya, None), M, label, only)
        assert all(torch.equal(got[False][n].isnan(), got[True][n].isnan()) for n in NAMES)


# ------------------------------------------------------------------------------------------------ autograd wrappers
@pytest.mark.parametrize("c", [1.0, 2.5])
@pytest.mark.parametrize("v_2d", [True, False])
@pytest.mark.parametrize("M", [3, 1025])
@pytest.mark.parametrize("packed", [False, True])
def test_loss_autograd_wrappers_scale_the_kernels_gradients(H, packed, M, v_2d, c):
    """``ppo_loss`` / ``ppo_loss_packed``: the value is the loss scalar, ``(c * loss).backward()`` leaves c x the kernel's three gradients
    (one rounding: rtol 1e-6 on the product) in the shapes of the leaves, ``out_scalars=`` receives the nine scalars."""
    gpu = _case(M)["gpu"]
    h = R.HYPERS[0]
    direct = R.kernel_run(gpu, h, 1, 1, packed)
    nl, en = gpu["newlogp"].clone().requires_grad_(), gpu["entropy"].clone().requires_grad_()
    nv = (gpu["newv"].reshape(M, 1) if v_2d else gpu["newv"]).clone().requires_grad_()
    out = torch.full((H.N_SCALARS,), float("nan"), device="cuda")
    if packed:
        loss = H.ppo_loss_packed(nl, nv, en, gpu["rec"], h["clip"], h["ent_coef"], h["vf_coef"], True, 1, out_scalars=out)
    else:
        ol, adv, ret, ov = (gpu["rec"][:, k].contiguous() for k in range(4))
        loss = H.ppo_loss(nl, nv, en, ol, adv, ov, ret, h["clip"], h["ent_coef"], h["vf_coef"], True, 1, out_scalars=out)
    assert loss.shape == () and torch.equal(loss, direct["scalars"][H.S_LOSS]) and torch.equal(out, direct["scalars"])
    (c * loss).backward()
    for leaf, n in ((nl, "g_newlogp"), (nv, "g_newv"), (en, "g_entropy")):
        assert leaf.grad.shape == leaf.shape, (n, leaf.grad.shape, leaf.shape)
        torch.testing.assert_close(leaf.grad.reshape(-1), c * direct[n], rtol=1e-6, atol=0.0)
    if c == 1.0:
        assert torch.equal(nl.grad, direct["g_newlogp"])


@pytest.mark.parametrize("M", [3, 1025])
def test_loss_surrogate_identity_of_the_per_sample_gradients(H, M):
    """What policies.py builds from the raw per-sample gradient: ``(lp * g_lp).sum() - (lp.detach() * g_lp).sum() + sc[S_PG]`` has the
    value ``pg`` (the two sums are the same computation on the same bits) and the gradient ``g_lp``."""
    gpu = _case(M)["gpu"]
    got = R.kernel_run(gpu, R.HYPERS[0], 1, 0, False)
    lp = gpu["newlogp"].clone().requires_grad_()
    s = (lp * got["g_newlogp"]).sum() - (lp.detach() * got["g_newlogp"]).sum() + got["scalars"][H.S_PG]
    assert torch.equal(s.detach(), got["scalars"][H.S_PG])
    s.backward()
    assert torch.equal(lp.grad, got["g_newlogp"])


# ------------------------------------------------------------------------------------------------ workspace
def test_loss_workspace_reuse_leaks_no_stale_partial(H):
    """M = 262145 and then M = 3 on one device workspace: bit-equal to M = 3 on a workspace whose every byte was 0xFF (NaN doubles) and on
    one of zeros.  A stale statistic partial, loss partial or mean / std stash that leaked into the small call would show."""
    small, big = _case(3), _case(262145)
    lib = H._lib.load()
    dev = small["gpu"]["newlogp"].device
    key = ("loss", dev.index if dev.index is not None else torch.cuda.current_device())
    for na, vm in ((1, 1), (0, 2)):
        runs = []
        for fill in (0xFF, 0x00):
            H._ws_cache[key] = torch.full((lib.aurppo_loss_workspace_bytes(3),), fill, dtype=torch.uint8, device=dev)
            for packed in (False, True):
                runs.append(R.kernel_run(small["gpu"], R.HYPERS[0], na, vm, packed))
        for packed in (False, True):
            R.kernel_run(big["gpu"], R.HYPERS[0], na, vm, packed)
            runs.append(R.kernel_run(small["gpu"], R.HYPERS[0], na, vm, packed))
        torch.cuda.synchronize()
        for r in runs[1:]:
            assert _bits_equal(runs[0], r)
        ref, Y = _ref(small, 0, na, vm)
        R.check(runs[-1], ref, Y, 3, f"after-M262145-{'norm' if na else 'raw'}-v{vm}")
