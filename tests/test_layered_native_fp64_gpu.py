"""GPU: the native layered PPO step (hip_ops.mlp_layered_step_native -> aurppo_mlp_layered_step_f32) and the minibatch call behind it
(hip_ops.mlp_layered_minibatch -> aurppo_mlp_layered_minibatch_f32).

T1  every case of tests/layered_cases.py and every step case of tests/layered_ragged_cases.py passes ``ref64.check_step`` unchanged
    (same inputs, yardstick and bars as tests/test_layered_fp64_gpu.py); everything but the lower layers' bias gradients -- which come
    out of the weight-gradient kernel instead of a column sum -- is ``mlp_layered_step``'s bit for bit (at L = 1 the whole gradient);
    nothing past ``n_params`` is written; a second launch gives the same bits.
T2  ``mlp_layered_minibatch`` equals the native step followed by ``clip_adam_`` in every bit of parameters, moments, step count, norm,
    gradient and scalars, at warm moments and t = 1000.
T3  AURPPO_ESHAPE before any launch for the shapes outside the limits."""
import ctypes as C

import pytest
import torch

from tests import layered_cases as LC
from tests import layered_ragged_cases as LR
from tests import ref64 as R
from tests import test_layered_ragged_fp64_gpu as LRG

pytestmark = pytest.mark.gpu

ESHAPE = -2
CASES = LC.CASES + LR.STEP_CASES
IDS = LC.IDS + LR.STEP_IDS
WORST = {}


def _lower_bias_mask(lay):
    """True at the bucket positions of the bias gradients the native step takes inside k_linear_wgrad: layers 0 .. L - 2, both nets."""
    L, Hd, off = lay["num_layers"], lay["hidden"], lay["offsets"]
    mask = torch.zeros(lay["n_params"], dtype=torch.bool, device="cuda")
    for net in range(2):
        for l in range(L - 1):
            o = off[net * 2 * (L + 1) + 2 * l + 1]
            mask[o:o + Hd] = True
    return mask


def _run(fn, obs, act, rec, idx, bucket, lay, c):
    g = torch.full((bucket.flat_grad.numel() + 64,), float("nan"), device="cuda")
    sc = fn(obs, act, rec, idx, bucket.flat_param, lay, g, R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    torch.cuda.synchronize()
    return sc.clone(), g          # (adv_std of a one-sample minibatch is NaN)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_native_step_matches_fp64_and_the_python_route(c):
    data = R.build_case(c)
    ref = R.reference_step(c, data)
    data["ref"] = ref
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    H, _pol, bucket, lay = LRG._policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    n = lay["n_params"]
    sc, g = _run(H.mlp_layered_step_native, obs, act, rec, idx, bucket, lay, c)
    sc2, g2 = _run(H.mlp_layered_step_native, obs, act, rec, idx, bucket, lay, c)
    assert bool(torch.isnan(g[n:]).all()), "the step wrote past n_params"
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    assert torch.equal(g[:n], g2[:n]) and same(sc, sc2), "two launches differ"
    sc_py, g_py = _run(H.mlp_layered_step, obs, act, rec, idx, bucket, lay, c)
    lower = _lower_bias_mask(lay)
    assert int(lower.sum()) == 2 * (c.layers - 1) * c.hidden
    assert same(sc, sc_py), "the nine scalars differ from mlp_layered_step's"
    assert torch.equal(g[:n][~lower], g_py[:n][~lower]), "a gradient outside the lower layers' biases differs from mlp_layered_step's"
    gm, _sm, rg, _rs = R.check_step(c, sc, g[:n], ref, Y, Ys, "layered native: aurppo_mlp_layered_step_f32")
    low = [m for name, m in gm.items() if name.endswith(".bias") and int(name.split(".")[2]) < 2 * (c.layers - 1)]
    assert len(low) == 2 * (c.layers - 1)
    if low and Y > 0:
        WORST[R.case_id(c)] = max(low) / Y
        print(f"lower-layer bias gradients: worst {max(low):.3e} = {max(low) / Y:.2f} x Y; worst of the cases so far {max(WORST.values()):.2f} x Y")


def _warm(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = 0.01 * torch.randn(n, device="cuda", generator=g)
    v = 1e-4 * torch.rand(n, device="cuda", generator=g)
    return m, v


@pytest.mark.parametrize("c", [R._mk("layered", 64, 1, 144, 6, True, 1, False, 1),
                               R._mk("layered", 256, 2, 17, 6, True, 257, True, 1),
                               R._mk("layered", 160, 3, 144, 6, False, 65, True, 1)], ids=["1x64-D144-M1", "2x256-D17-M257", "3x160-cat-M65"])
def test_minibatch_equals_step_then_clip_adam(c):
    data = R.build_case(c)
    H, _pol, bucket, lay = LRG._policy(c.hidden, c.layers, c.D, c.A, c.cont, data["sd"])
    obs, act, rec, idx = R.gpu_inputs(c, data)
    N = lay["n_params"]                             # buffers of exactly n_params floats: clip_adam_ then covers [0, n_params) too
    p0 = bucket.flat_param[:N].clone()
    knobs = (R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    lr = torch.tensor([2.5e-4], device="cuda")
    outs = []
    for fused in (False, True):
        p, grad = p0.clone(), torch.full((N,), float("nan"), device="cuda")
        m, v = _warm(N, c.seed)
        t, norm, sc = torch.tensor([1000.0], device="cuda"), torch.full((1,), float("nan"), device="cuda"), torch.empty(9, device="cuda")
        if fused:
            H.mlp_layered_minibatch(obs, act, rec, idx, p, lay, grad, *knobs, sc, m, v, lr, t, 0.5, (0.9, 0.999), 1e-5, norm)
        else:
            H.mlp_layered_step_native(obs, act, rec, idx, p, lay, grad, *knobs, sc)
            H.clip_adam_(p, grad, m, v, lr, t, 0.5, betas=(0.9, 0.999), eps=1e-5, out_norm=norm)
        torch.cuda.synchronize()
        outs.append(dict(p=p, grad=grad, m=m, v=v, t=t, norm=norm, sc=torch.nan_to_num(sc, nan=-7.0)))
    a, b = outs
    assert float(a["t"]) == 1001.0 and bool(torch.isfinite(a["p"]).all()) and not torch.equal(a["p"], p0)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between the minibatch call and step + clip_adam_"


@pytest.mark.parametrize("hidden,A,cont,M", [(48, 6, True, 65), (1056, 6, True, 65), (256, 17, True, 65), (256, 1, False, 65), (256, 6, True, 0)],
                         ids=["hidden48", "hidden1056", "A17", "cat-A1", "M0"])
@pytest.mark.parametrize("call", ["step", "minibatch"])
def test_shapes_outside_the_limits_are_refused_before_any_launch(hidden, A, cont, M, call):
    from aur_ppo_amd import _lib
    lib = _lib.load()
    D, L, B = 16, 2, 128
    n = 2 * (D * hidden + hidden + hidden * hidden + hidden) + (A + 1) * (hidden + 1) + A
    lay, pos = [], 0
    for out in (A, 1):
        for rows, cols in ((hidden, D), (hidden, hidden), (out, hidden)):
            lay += [pos, pos + rows * cols]
            pos += rows * cols + rows
    lay.append(pos)
    assert pos + A == n and len(lay) == 4 * (L + 1) + 1
    if cont:            # (the size function does not know the head's kind: a Gaussian head of one action is a shape it takes)
        assert lib.aurppo_mlp_layered_step_workspace_bytes(M, D, A, hidden, L) == 0
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    obs, act, rec, idx = f(B, D), f(B, A), f(B, 4), torch.zeros(max(M, 1), dtype=torch.int32, device="cuda")
    p, grad, sc, ws = f(n), f(n), f(9), torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    m, v, lr, t, norm = f(n), f(n), f(1), f(1), f(1)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    args = [ptr(obs), ptr(act), ptr(rec), ptr(idx), M, D, A, int(cont), hidden, L, ptr(p), (C.c_int * len(lay))(*lay), n, ptr(grad),
            0.2, 0.01, 0.5, 1, 1, ptr(sc)]
    tail = [ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    if call == "step":
        rc = lib.aurppo_mlp_layered_step_f32(*args, *tail)
    else:
        rc = lib.aurppo_mlp_layered_minibatch_f32(*args, ptr(m), ptr(v), 0.5, ptr(lr), ptr(t), 0.9, 0.999, 1e-5, ptr(norm), *tail)
    torch.cuda.synchronize()
    assert rc == ESHAPE, (rc, lib.aurppo_last_error())
    for x in (p, grad, sc, m, v, t, norm):
        assert bool(torch.isnan(x).all()), "something was launched"
