"""CPU: the host layer of K11p (aurppo_conv3x3_pool_f32: a hidden encoder block's convolution, bias, ReLU and 2 x 2 max-pool in one
launch).  (1) The binding exists with the header's prototype.  (2) ``conv3x3_pool_ok`` / ``conv3x3_pool_supported`` over the GPU suite's
shapes (tests/conv_pool_cases.py), refusals included, and the restated launch plan against the shapes' comments.  (3) What
``hip_ops.conv3x3_pool`` hands to the library, forward and backward, equals tests/transcripts/conv_pool_calls.json (the recorder of
tests/test_hip_ops_calls.py, imported).  (4) ``base_encoder._blocks`` and ``equiv._Block`` route through it only with
AURPPO_K11_POOL=1: unset or "0", the calls are today's.

Re-record with ``python tests/test_conv_pool_host.py`` and READ THE DIFF whenever the C signature or the wrapper's argument list changes."""
import importlib.util
import json
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import conv_pool_cases as CP                # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "conv_pool_calls.json")
PROTOTYPE = ("int aurppo_conv3x3_pool_f32(const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int Ci, "
             "int Co, int H, int W, int pad, void* wop_ws, void* stream);")


# ------------------------------------------------------------------ (1) the binding
def test_the_header_declares_the_prototype_and_the_binding_carries_it():
    import ctypes as C
    import __graft_entry__ as g
    with open(os.path.join(ROOT, "include", "aurppo.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert PROTOTYPE in header
    assert "aurppo_conv3x3_pool_f32" in TC._lib.SYMBOLS
    g.build()
    fn = TC._lib.load().aurppo_conv3x3_pool_f32
    assert list(fn.argtypes) == [C.c_void_p] * 5 + [C.c_int32] * 6 + [C.c_void_p] * 2
    assert fn.restype in (C.c_int, C.c_int32)


# ------------------------------------------------------------------ (2) the shape rule
def _gpu_like(shape, dtype=torch.float32, cuda=True):
    return types.SimpleNamespace(shape=tuple(shape), dtype=dtype, is_cuda=cuda, dim=lambda: len(shape))


def _x(s, **kw):
    return _gpu_like((s[0], s[1], s[3], s[4]), **kw)


@pytest.mark.parametrize("s", CP.SHAPES, ids=CP.IDS)
def test_the_plan_is_what_the_shape_list_says(s):
    assert CP.plan(*s) == CP.CLAIMS[s]


def test_conv3x3_pool_ok_over_the_shape_list(monkeypatch):
    # at the library's thresholds none of the suite's small shapes is worth a launch
    for s in CP.SHAPES + [CP.REFUSED]:
        assert not H.conv3x3_pool_ok(_x(s), s[1], s[2], s[5])
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 0)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 0)
    for s in CP.SHAPES:
        # conv3x3_ok's rule: whole 32-channel blocks (the C entry point itself takes any channel count)
        assert H.conv3x3_pool_ok(_x(s), s[1], s[2], s[5]) == (s[2] % 32 == 0), s
    took = [s for s in CP.SHAPES if s[2] % 32 == 0]
    assert len(took) >= 4
    s = took[0]
    assert not H.conv3x3_pool_ok(_x(s, cuda=False), s[1], s[2], s[5])
    assert not H.conv3x3_pool_ok(_x(s, dtype=torch.float64), s[1], s[2], s[5])
    assert not H.conv3x3_pool_ok(_x(s), s[1] + 16, s[2], s[5])                 # not x's channel count
    assert not H.conv3x3_pool_ok(_gpu_like((1, 24, 8, 8)), 24, 32, 1)          # no whole k-step
    assert not H.conv3x3_pool_ok(_x(s), s[1], s[2], 3)
    # no whole window: Hp = 0 / Wp = 0, whatever the thresholds
    assert not H.conv3x3_pool_ok(_gpu_like((5, 48, 1, 1)), 48, 32, 1)
    assert not H.conv3x3_pool_ok(_gpu_like((5, 48, 8, 3)), 48, 32, 0)
    assert H.conv3x3_pool_ok(_gpu_like((5, 48, 8, 4)), 48, 32, 0)


def test_the_pixel_count_is_that_of_the_whole_windows(monkeypatch):
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 1 << 40)
    # 21 x 21: 441 output pixels an image, 400 of them in windows
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 400 * 7)
    x = _gpu_like((7, 32, 21, 21))
    assert H.conv3x3_pool_ok(x, 32, 64, 1)
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 400 * 7 + 1)
    assert not H.conv3x3_pool_ok(x, 32, 64, 1) and H.conv3x3_ok(x, 32, 64, 1)
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 1 << 40)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 11)          # ceil(2800 / 256) = 11 workgroups x one 128-channel group
    assert H.conv3x3_pool_ok(x, 32, 64, 1)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 12)
    assert not H.conv3x3_pool_ok(x, 32, 64, 1)


def test_the_policy_blocks_are_taken_at_the_library_thresholds():
    for B, ci, co, hw in ((8192, 16, 32, 64), (8192, 32, 64, 32), (8192, 64, 128, 16), (8192, 32, 64, 21)):
        conv = torch.nn.Conv2d(ci, co, 3, padding=1)
        assert H.conv3x3_pool_supported(_gpu_like((B, ci, hw, hw)), conv)


def test_conv3x3_pool_supported_is_conv3x3_supported_s_module_rule(monkeypatch):
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 0)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 0)
    x = _gpu_like((2, 16, 8, 8))
    nn = torch.nn
    assert H.conv3x3_pool_supported(x, nn.Conv2d(16, 32, 3, padding=1))
    assert H.conv3x3_pool_supported(x, nn.Conv2d(16, 32, 3, padding=0))
    for bad in (nn.Conv2d(16, 32, 3, padding=1, stride=2), nn.Conv2d(16, 32, 3, padding=2, dilation=2),
                nn.Conv2d(16, 32, 3, padding=1, groups=2), nn.Conv2d(16, 32, 5, padding=1), nn.Conv2d(16, 32, 3, padding=(1, 2)),
                nn.Conv2d(16, 32, 3, padding=1, padding_mode="reflect"), nn.Conv2d(16, 48, 3, padding=1), nn.Conv2d(32, 32, 3, padding=1)):
        assert not H.conv3x3_pool_supported(x, bad), bad


# ------------------------------------------------------------------ (3) what the host layer hands to the library
CASES = {}


def _pool_case(Ci, with_bias):
    def run(h):
        Bn, Co, Hh, Ww, pad = 2, 64, 5, 7, 1          # 5 x 7 -> 2 x 3: an odd row and column that no window holds
        x, w = h.t("x", Bn, Ci, Hh, Ww).requires_grad_(True), h.t("w", Co, Ci, 3, 3).requires_grad_(True)
        bias = h.t("bias", Co).requires_grad_(True) if with_bias else None
        y = H.conv3x3_pool(x, w, bias, pad)
        assert y.shape == (Bn, Co, 2, 3)
        h.name("y", y)
        mask = y.grad_fn.saved_tensors[2]
        assert mask.dtype == torch.uint8 and mask.shape == y.shape
        h.name("mask", mask)
        y.backward(h.t("dy", Bn, Co, 2, 3))
        h.name("dx", x.grad)
        assert x.grad.shape == x.shape and w.grad.shape == w.shape
        assert (bias.grad.shape == (Co,)) if with_bias else True
    return run


CASES["conv3x3_pool/bias/dx_library"] = _pool_case(32, True)
CASES["conv3x3_pool/bias/dx_aten"] = _pool_case(16, True)
CASES["conv3x3_pool/no_bias/dx_library"] = _pool_case(32, False)


def run_case(name, setattr_, bound=None):
    h = TC.Harness(bound)
    h.install(setattr_)
    CASES[name](h)
    return json.loads(json.dumps(h.transcript()))


def _recorded():
    with open(TRANSCRIPT) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(_recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_match_the_recorded_transcript(name, monkeypatch):
    got, want = run_case(name, monkeypatch.setattr), _recorded()[name]
    assert len(got) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs"
    assert len(got) == len(want)


def test_every_call_fits_the_bound_argtypes(monkeypatch):
    import __graft_entry__ as g
    g.build()
    bound = TC._lib.load()
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


def test_the_backward_is_k9_s_then_conv3x3_s(monkeypatch):
    """The fused function's backward: K9's backward on the saved mask, then the very calls ``conv3x3``'s backward makes."""
    fused = [c[0] for c in run_case("conv3x3_pool/bias/dx_library", monkeypatch.setattr)]
    h = TC.Harness()
    with monkeypatch.context() as m:
        h.install(m.setattr)
        x, w = h.t("x", 2, 32, 5, 7).requires_grad_(True), h.t("w", 64, 32, 3, 3).requires_grad_(True)
        H.bias_relu_pool2(H.conv3x3(x, w, 1), h.t("bias", 64).requires_grad_(True)).backward(h.t("dy", 2, 64, 2, 3))
    pair = [c[0] for c in h.calls]
    assert fused[:3] == ["aurppo_conv3x3_wop_bytes", "_workspace", "aurppo_conv3x3_pool_f32"]
    assert pair[:4] == ["aurppo_conv3x3_wop_bytes", "_workspace", "aurppo_conv3x3_f32", "aurppo_bias_relu_pool2_fwd_f32"]
    assert fused[3:] == pair[4:] and fused[3] == "aurppo_bias_relu_pool2_bwd_f32"


# ------------------------------------------------------------------ (4) the callers
class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the encoders take their GPU routes, the stand-ins below compute them with torch."""
    is_cuda = True


def _fresh(name, env, monkeypatch):
    """aur_ppo_amd/<name>.py executed anew under ``AURPPO_K11_POOL = env`` (None: unset), outside sys.modules: its switches are read at
    import, and the modules the rest of the suite holds stay as they are."""
    if env is None:
        monkeypatch.delenv("AURPPO_K11_POOL", raising=False)
    else:
        monkeypatch.setenv("AURPPO_K11_POOL", env)
    spec = importlib.util.spec_from_file_location(f"aur_ppo_amd.{name}", os.path.join(ROOT, "aur_ppo_amd", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Recorder:
    """Stands in for the launching functions of ``hip_ops`` (the shape rules stay the real ones): records (name, shapes), computes with torch."""

    def __init__(self, monkeypatch):
        self.calls = []
        F = torch.nn.functional

        def conv3x3(x, w, pad):
            self.calls.append(("conv3x3", tuple(x.shape), tuple(w.shape), int(pad)))
            return F.conv2d(x, w, None, padding=pad)

        def brp(z, bias=None, scale=None, plane=None):
            self.calls.append(("bias_relu_pool2", tuple(z.shape), bias is not None, scale is not None, plane is not None))
            if plane is not None:
                z = z + scale.reshape(-1, 1, 1, 1) * plane
            if bias is not None:
                z = z + bias.reshape(1, -1, 1, 1)
            return F.max_pool2d(torch.relu(z), 2)

        def pool(x, w, bias, pad):
            self.calls.append(("conv3x3_pool", tuple(x.shape), tuple(w.shape), bias is not None, int(pad)))
            z = F.conv2d(x, w, None, padding=pad)
            if bias is not None:
                z = z + bias.reshape(1, -1, 1, 1)
            return F.max_pool2d(torch.relu(z), 2)

        def first_block(obs, state, w, bias):
            self.calls.append(("first_block", tuple(obs.shape), tuple(w.shape)))
            c = obs.shape[1]
            z = F.conv2d(obs, w[:, :c], None, padding=1)
            z = z + state.reshape(-1, 1, 1, 1) * F.conv2d(torch.ones_like(obs[:1, :1]), w[:, c:c + 1], None, padding=1)
            return F.max_pool2d(torch.relu(z + bias.reshape(1, -1, 1, 1)), 2)

        for n, f in (("conv3x3", conv3x3), ("bias_relu_pool2", brp), ("conv3x3_pool", pool), ("first_block", first_block)):
            monkeypatch.setattr(H, n, f)
        monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 0)
        monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 0)

    def names(self):
        return [c[0] for c in self.calls]


def _fused_pairs(names):
    """``names`` with every conv3x3 that a bias_relu_pool2 follows folded into one conv3x3_pool."""
    out, i = [], 0
    while i < len(names):
        if names[i] == "conv3x3" and i + 1 < len(names) and names[i + 1] == "bias_relu_pool2":
            out.append("conv3x3_pool")
            i += 2
        else:
            out.append(names[i])
            i += 1
    return out


def _obs(size, ch=2):
    g = torch.Generator().manual_seed(size)
    return torch.randn(1, ch, size, size, generator=g).as_subclass(_OnGpu)


# today's calls: the first block's convolution is the library's (2 input channels), every later (Conv2d, ReLU, MaxPool2d) triple is
# conv3x3 + bias_relu_pool2, the convolutions without a pool behind them conv3x3 alone
BASE_TODAY = {84: ["bias_relu_pool2"] + ["conv3x3", "bias_relu_pool2"] * 3 + ["conv3x3"] * 2,
              128: ["bias_relu_pool2"] + ["conv3x3", "bias_relu_pool2"] * 3 + ["conv3x3", "conv3x3", "bias_relu_pool2", "conv3x3"]}
BASE_FUSED = {84: 3, 128: 4}


@pytest.mark.parametrize("size", [84, 128])
@pytest.mark.parametrize("env", [None, "0", "1"])
def test_base_encoder_blocks(size, env, monkeypatch):
    mod = _fresh("base_cnns", env, monkeypatch)
    assert mod.base_encoder.fused_block == (env == "1")
    torch.manual_seed(0)
    enc = mod.base_encoder((2, size, size), out_dim=128)
    rec = _Recorder(monkeypatch)
    x = _obs(size)
    with torch.no_grad():
        out = enc(x)
        ref = enc.conv(x.as_subclass(torch.Tensor))           # the stock modules on a plain tensor
    assert torch.allclose(out.as_subclass(torch.Tensor), ref, rtol=1e-5, atol=1e-6)
    want = BASE_TODAY[size] if env != "1" else _fused_pairs(BASE_TODAY[size])
    assert rec.names() == want
    assert rec.names().count("conv3x3_pool") == (BASE_FUSED[size] if env == "1" else 0)
    for c in rec.calls:
        if c[0] == "conv3x3_pool":                # the module's own weight, its bias, its padding
            assert c[3] is True and c[2][2:] == (3, 3) and c[4] in (0, 1)
    # the split first block (the state plane rides in K9, or the whole block is K10): never the fused route, whatever the switch
    state = torch.tensor([[1.0]])
    for fused_first in (True, False):
        rec.calls.clear()
        enc.fused_first = fused_first
        with torch.no_grad():
            out2 = enc.forward_split(_obs(size, 1), state)
        head = ["first_block"] if fused_first else ["bias_relu_pool2"]
        assert rec.names() == head + want[1:]
        if not fused_first:
            assert rec.calls[0][2:] == (True, True, True)          # bias, scale and plane: K9's tail, kept
        assert out2.shape == out.shape
    # every switch of its own still holds: without K11 there is no K11p
    rec.calls.clear()
    enc.fused_conv = False
    with torch.no_grad():
        enc(x)
    assert set(rec.names()) == {"bias_relu_pool2"}


EQUIV_TODAY = ["bias_relu_pool2"] + ["conv3x3", "bias_relu_pool2"] * 3 + ["conv3x3", "conv3x3", "bias_relu_pool2", "conv3x3"]


@pytest.mark.parametrize("env", [None, "0", "1"])
def test_equivariant_blocks(env, monkeypatch):
    mod = _fresh("equiv", env, monkeypatch)
    assert mod._Block.fused_block == (env == "1")
    torch.manual_seed(0)
    enc = mod.EquivariantEncoder(2, 32, 128)      # 16 - 32 - 64 - 128 - 256 - 128 - 128 channels
    rec = _Recorder(monkeypatch)
    x = _obs(128)
    with torch.no_grad():
        out = enc(x)
    want = EQUIV_TODAY if env != "1" else _fused_pairs(EQUIV_TODAY)
    assert rec.names() == want
    assert rec.names().count("conv3x3_pool") == (4 if env == "1" else 0)
    if env == "1":
        pools = [c for c in rec.calls if c[0] == "conv3x3_pool"]
        # the EXPANDED filter bank and bias: four channels per regular field
        assert [c[2][:2] for c in pools] == [(32, 16), (64, 32), (128, 64), (128, 256)] and all(c[3] for c in pools)
        assert [c[4] for c in pools] == [1, 1, 1, 0]
    rec.calls.clear()
    for blk in enc.conv:
        blk.fused_pool = False                     # the stock route: what the fused one must equal
    with torch.no_grad():
        ref = enc(x)
    assert torch.allclose(out.as_subclass(torch.Tensor), ref.as_subclass(torch.Tensor), rtol=1e-5, atol=1e-6)


if __name__ == "__main__":
    class _Patch:
        def __init__(self):
            self.undo = []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

        def restore(self):
            for obj, name, old in reversed(self.undo):
                setattr(obj, name, old)

    result = {}
    for case_name in sorted(CASES):
        patch = _Patch()
        try:
            result[case_name] = run_case(case_name, patch.setattr)
        finally:
            patch.restore()
    os.makedirs(os.path.dirname(TRANSCRIPT), exist_ok=True)
    with open(TRANSCRIPT, "w") as f:
        f.write(TC._dump(result))
    print(f"{len(result)} cases, {sum(len(v) for v in result.values())} calls -> {TRANSCRIPT}")
