"""CPU: the host layer of K11x (hidden activations kept as bf16 planes; include/aurppo.h holds the layout).  (1) The header declares
each new symbol with its prototype and the binding carries it.  (2) ``aurppo_planes_bytes`` over good and refused shapes.  (3) The numpy
restatement of the split that the GPU suite compares the kernels with (tests/conv_planes_cases.py) joins back to its input exactly.
(4) What the new ``hip_ops`` entry points hand to the library, forward and backward, equals tests/transcripts/conv_planes_calls.json
(the recorder of tests/test_hip_ops_calls.py, imported).  (5) ``base_encoder`` carries planes from block to block only with
AURPPO_K11_PLANES=1, and each consumer receives its predecessor's.

Re-record with ``python tests/test_conv_planes_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import conv_planes_cases as XP              # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "conv_planes_calls.json")
VP, I32 = C.c_void_p, C.c_int32
PROTOTYPES = {
    "aurppo_planes_bytes": ("size_t aurppo_planes_bytes(int B, int C, int H, int W);", [I32] * 4),
    "aurppo_split_planes_f32": ("int aurppo_split_planes_f32(const float* x, uint16_t* xp, int B, int C, int H, int W, void* stream);",
                                [VP] * 2 + [I32] * 4 + [VP]),
    "aurppo_conv3x3_planes_f32": ("int aurppo_conv3x3_planes_f32(const uint16_t* xp, const float* w, float* z, int B, int Ci, int Co, int H, "
                                  "int W, int pad, void* wop_ws, void* stream);", [VP] * 3 + [I32] * 6 + [VP] * 2),
    "aurppo_conv3x3_pool_planes_f32": ("int aurppo_conv3x3_pool_planes_f32(const void* x_or_xp, int x_is_planes, const float* w, "
                                       "const float* bias, float* y, uint8_t* mask, uint16_t* yp_or_null, int B, int Ci, int Co, int H, "
                                       "int W, int pad, void* wop_ws, void* stream);", [VP, I32] + [VP] * 5 + [I32] * 6 + [VP] * 2),
    "aurppo_first_block_planes_fwd_f32": ("int aurppo_first_block_planes_fwd_f32(const float* obs, const float* w, const float* bias, "
                                          "const float* state, float* y, uint8_t* mask, uint16_t* yp, int B, int Ci, int Co, int H, int W, "
                                          "void* stream);", [VP] * 7 + [I32] * 5 + [VP]),
}


# ------------------------------------------------------------------ (1) the bindings
@pytest.fixture(scope="module")
def bound():
    import __graft_entry__ as g
    g.build()
    return TC._lib.load()


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_the_header_declares_the_prototype_and_the_binding_carries_it(name, bound):
    proto, argtypes = PROTOTYPES[name]
    with open(os.path.join(ROOT, "include", "aurppo.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert proto in header
    assert name in TC._lib.SYMBOLS
    fn = getattr(bound, name)
    assert list(fn.argtypes) == argtypes
    assert fn.restype is C.c_size_t if name == "aurppo_planes_bytes" else fn.restype in (C.c_int, C.c_int32)


def test_the_header_documents_the_layout_once():
    with open(os.path.join(ROOT, "include", "aurppo.h")) as f:
        header = f.read()
    assert header.count("THE PLANES LAYOUT") == 1
    assert "xp[B][C / 8][3][H * W][8]" in header


# ------------------------------------------------------------------ (2) the size
def test_planes_bytes(bound):
    f = bound.aurppo_planes_bytes
    assert f(1, 8, 1, 1) == 48
    assert f(2, 16, 3, 5) == 6 * 2 * 16 * 15
    assert f(8192, 16, 64, 64) == 6 * 8192 * 16 * 64 * 64           # 3 GiB: past 32 bits
    assert f(2048, 128, 8, 8) == 6 * 2048 * 128 * 64
    for bad in ((1, 12, 4, 4), (1, 4, 4, 4), (1, 7, 1, 1), (0, 8, 4, 4), (1, 0, 4, 4), (1, 8, 0, 4), (1, 8, 4, 0), (-1, 8, 4, 4), (1, -8, 4, 4)):
        assert f(*bad) == 0, bad


# ------------------------------------------------------------------ (3) the restated split
def test_the_restated_split_joins_back_exactly():
    x = XP.wide_range(100000, seed=7)
    assert float(np.abs(x).min()) >= 2.0 ** -100 and float(np.abs(x).max()) <= 2.0 ** 100
    p0, p1, p2 = XP.split3(x)
    assert np.array_equal(XP.join3(p0, p1, p2).view(np.uint32), x.view(np.uint32))
    # plane 0 is the value rounded to nearest even, and the residual planes are small: 8 bits each
    v0 = (p0.astype(np.uint32) << 16).view(np.float32)
    assert float(np.max(np.abs(x - v0) / np.abs(x))) <= 2.0 ** -8
    z = np.array([0.0, -0.0], dtype=np.float32)
    q0, q1, q2 = XP.split3(z)
    assert q0.tolist() == [0x0000, 0x8000] and q1.tolist() == [0, 0] and q2.tolist() == [0, 0]
    # (-0.0's sign lives in plane 0; summed with the +0.0 residual planes it is +0.0 under round-to-nearest: equal in value, and the
    # matrix pipe multiplies plane 0, so the sign is not lost to the convolution)
    assert np.array_equal(XP.join3(q0, q1, q2), z)


def test_the_restated_rounding_is_to_nearest_even():
    f = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)
    assert XP.bf16_rne(f(0x3F808000))[0][0] == 0x3F80          # a tie: to the even neighbour below
    assert XP.bf16_rne(f(0x3F818000))[0][0] == 0x3F82          # a tie: to the even neighbour above
    assert XP.bf16_rne(f(0x3F808001))[0][0] == 0x3F81
    assert XP.bf16_rne(f(0x7F800000))[0][0] == 0x7F80 and XP.bf16_rne(f(0xFF800000))[0][0] == 0xFF80
    assert XP.bf16_rne(f(0x7F7FFFFF))[0][0] == 0x7F80          # the largest float rounds to infinity
    assert XP.bf16_rne(f(0xFFC00001))[0][0] == 0x7FC0


def test_the_restated_layout():
    x = np.arange(2 * 16 * 2 * 3, dtype=np.float32).reshape(2, 16, 2, 3) * 1.001
    p = XP.planes_np(x)
    assert p.shape == (2, 2, 3, 6, 8) and p.dtype == np.uint16
    for (b, c, yy, xx) in ((0, 0, 0, 0), (1, 9, 1, 2), (1, 15, 0, 1)):
        want = [int(q[0]) for q in XP.split3(np.array([x[b, c, yy, xx]], dtype=np.float32))]
        assert [int(p[b, c // 8, pl, yy * 3 + xx, c % 8]) for pl in range(3)] == want


# ------------------------------------------------------------------ (4) what the host layer hands to the library
CASES = {}


def _planes(h, name, x):
    B, Cc, Hh, Ww = x.shape
    return h.name(name, torch.zeros((B, Cc // 8, 3, Hh * Ww, 8), dtype=torch.int16))


def _split_case(h):
    x = h.t("x", 2, 16, 5, 7)
    xp = H.split_planes(x)
    assert xp.dtype == torch.int16 and tuple(xp.shape) == (2, 2, 3, 35, 8)
    h.name("xp", xp)


def _conv_case(h):
    x, w = h.t("x", 2, 32, 5, 7).requires_grad_(True), h.t("w", 64, 32, 3, 3).requires_grad_(True)
    xp = _planes(h, "xp", x)
    z = H.conv3x3_planes(x, xp, w, 1)
    assert z.shape == (2, 64, 5, 7)
    h.name("z", z)
    z.backward(h.t("dz", 2, 64, 5, 7))
    h.name("dx", x.grad)
    assert x.grad.shape == x.shape and w.grad.shape == w.shape


def _pool_case(planes_in, want, with_bias=True, fp32_wrapper=False):
    def run(h):
        Bn, Ci, Co, Hh, Ww, pad = 2, 32, 64, 5, 7, 1
        x, w = h.t("x", Bn, Ci, Hh, Ww).requires_grad_(True), h.t("w", Co, Ci, 3, 3).requires_grad_(True)
        bias = h.t("bias", Co).requires_grad_(True) if with_bias else None
        xp = _planes(h, "xp", x) if planes_in else None
        y = H.conv3x3_pool(x, w, bias, pad) if fp32_wrapper else H.conv3x3_pool_planes(x, xp, w, bias, pad, want_planes=want)
        if want:
            y, yp = y
            assert yp.dtype == torch.int16 and tuple(yp.shape) == (Bn, Co // 8, 3, 6, 8) and not yp.requires_grad
            h.name("yp", yp)
        assert y.shape == (Bn, Co, 2, 3)
        h.name("y", y)
        saved = y.grad_fn.saved_tensors
        assert [tuple(t.shape) for t in saved] == [tuple(x.shape), tuple(w.shape), tuple(y.shape)]      # fp32 x, w and the mask: as K11p
        assert saved[2].dtype == torch.uint8
        h.name("mask", saved[2])
        y.backward(h.t("dy", Bn, Co, 2, 3))
        h.name("dx", x.grad)
        assert x.grad.shape == x.shape and w.grad.shape == w.shape
    return run


def _first_case(h):
    obs, state = h.t("obs", 2, 1, 8, 8), h.t("state", 2)
    w, bias = h.t("w", 16, 2, 3, 3).requires_grad_(True), h.t("bias", 16).requires_grad_(True)
    y, yp = H.first_block(obs, state, w, bias, want_planes=True)
    assert tuple(yp.shape) == (2, 2, 3, 16, 8) and yp.dtype == torch.int16 and not yp.requires_grad
    h.name("y", y)
    h.name("yp", yp)
    h.name("mask", y.grad_fn.saved_tensors[2])
    y.backward(h.t("dy", 2, 16, 4, 4))
    assert w.grad.shape == w.shape and bias.grad.shape == bias.shape


CASES["split_planes"] = _split_case
CASES["conv3x3_planes"] = _conv_case
CASES["conv3x3_pool_planes/in"] = _pool_case(True, False)
CASES["conv3x3_pool_planes/out"] = _pool_case(False, True)
CASES["conv3x3_pool_planes/in_out"] = _pool_case(True, True)
CASES["conv3x3_pool_planes/in_out/no_bias"] = _pool_case(True, True, with_bias=False)
CASES["conv3x3_pool_planes/neither"] = _pool_case(False, False)
CASES["first_block/planes"] = _first_case


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


def test_every_call_fits_the_bound_argtypes(monkeypatch, bound):
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


def test_planes_neither_in_nor_out_is_conv3x3_pool_call_for_call(monkeypatch):
    def transcript(run):
        h = TC.Harness()
        with monkeypatch.context() as m:
            h.install(m.setattr)
            run(h)
        return h.transcript()

    got = transcript(CASES["conv3x3_pool_planes/neither"])
    assert got == transcript(_pool_case(False, False, fp32_wrapper=True))
    assert [c[0] for c in got][:3] == ["aurppo_conv3x3_wop_bytes", "_workspace", "aurppo_conv3x3_pool_f32"]


def test_one_autograd_function_stands_behind_the_four_wrappers_and_one_behind_first_block(monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    x, w, bias = h.t("x", 2, 32, 5, 7).requires_grad_(True), h.t("w", 64, 32, 3, 3).requires_grad_(True), h.t("bias", 64)
    xp = _planes(h, "xp", x)
    outs = [H.conv3x3(x, w, 1), H.conv3x3_pool(x, w, bias, 1), H.conv3x3_planes(x, xp, w, 1), H.conv3x3_pool_planes(x, xp, w, bias, 1),
            H.conv3x3_pool_planes(x, None, w, bias, 1), H.conv3x3_pool_planes(x, xp, w, bias, 1, want_planes=True)[0]]
    kinds = {type(y.grad_fn) for y in outs}
    assert len(kinds) == 1 and None not in {y.grad_fn for y in outs}
    assert [len(y.grad_fn.saved_tensors) for y in outs] == [2, 3, 2, 3, 3, 3]
    obs, state = h.t("obs", 2, 1, 8, 8), h.t("state", 2)
    fw, fb = h.t("fw", 16, 2, 3, 3).requires_grad_(True), h.t("fb", 16).requires_grad_(True)
    first = [H.first_block(obs, state, fw, fb), H.first_block(obs, state, fw, fb, want_planes=False),
             H.first_block(obs, state, fw, fb, want_planes=True)[0]]
    assert len({type(y.grad_fn) for y in first}) == 1 and first[0].grad_fn is not None
    assert not kinds & {type(first[0].grad_fn)}


def test_the_backwards_are_the_fp32_functions(monkeypatch):
    """Behind its forward call, every planes function makes the very calls its fp32 sibling makes."""
    def names(run):
        h = TC.Harness()
        with monkeypatch.context() as m:
            h.install(m.setattr)
            run(h)
        return [c[0] for c in h.calls]

    def pool_f32(h):
        x, w = h.t("x", 2, 32, 5, 7).requires_grad_(True), h.t("w", 64, 32, 3, 3).requires_grad_(True)
        H.conv3x3_pool(x, w, h.t("bias", 64).requires_grad_(True), 1).backward(h.t("dy", 2, 64, 2, 3))

    def conv_f32(h):
        x, w = h.t("x", 2, 32, 5, 7).requires_grad_(True), h.t("w", 64, 32, 3, 3).requires_grad_(True)
        H.conv3x3(x, w, 1).backward(h.t("dz", 2, 64, 5, 7))

    def first_f32(h):
        w, bias = h.t("w", 16, 2, 3, 3).requires_grad_(True), h.t("bias", 16).requires_grad_(True)
        H.first_block(h.t("obs", 2, 1, 8, 8), h.t("state", 2), w, bias).backward(h.t("dy", 2, 16, 4, 4))

    for planes, f32, fwd in ((CASES["conv3x3_pool_planes/in_out"], pool_f32, ("aurppo_conv3x3_pool_planes_f32", "aurppo_conv3x3_pool_f32")),
                             (CASES["conv3x3_planes"], conv_f32, ("aurppo_conv3x3_planes_f32", "aurppo_conv3x3_f32")),
                             (CASES["first_block/planes"], first_f32, ("aurppo_first_block_planes_fwd_f32", "aurppo_first_block_fwd_f32"))):
        a, b = names(planes), names(f32)
        assert a.count(fwd[0]) == 1 and fwd[0] not in b          # (K11's mode 1 shares conv3x3_f32's name: it may follow in both)
        assert [fwd[1] if n == fwd[0] else n for n in a] == b


# ------------------------------------------------------------------ (5) the encoder
class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the encoder takes its GPU routes, the stand-ins below compute them with torch."""
    is_cuda = True


def _fresh(env, monkeypatch, pool_env=None):
    """aur_ppo_amd/base_cnns.py executed anew under ``AURPPO_K11_PLANES = env`` (None: unset), outside sys.modules."""
    for k, v in (("AURPPO_K11_PLANES", env), ("AURPPO_K11_POOL", pool_env)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    spec = importlib.util.spec_from_file_location("aur_ppo_amd.base_cnns", os.path.join(ROOT, "aur_ppo_amd", "base_cnns.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Recorder:
    """Stands in for the launching functions of ``hip_ops`` (the shape rules stay the real ones): records what each call was given, computes
    with torch, and hands out numbered tokens as planes so that a consumer's planes can be traced to their producer."""

    def __init__(self, monkeypatch):
        self.calls, self.made = [], {}
        F = torch.nn.functional

        def token(y):
            t = torch.tensor([len(self.made)], dtype=torch.int16)
            self.made[int(t)] = y
            return t

        def block(x, w, bias, pad):
            z = F.conv2d(x, w, None, padding=pad)
            if bias is not None:
                z = z + bias.reshape(1, -1, 1, 1)
            return F.max_pool2d(torch.relu(z), 2)

        def conv3x3(x, w, pad):
            self.calls.append(("conv3x3", tuple(x.shape), None, False))
            return F.conv2d(x, w, None, padding=pad)

        def conv3x3_planes(x, xp, w, pad):
            assert self.made[int(xp)] is x, "the planes are not this input's"
            self.calls.append(("conv3x3_planes", tuple(x.shape), int(xp), False))
            return F.conv2d(x, w, None, padding=pad)

        def brp(z, bias=None, scale=None, plane=None):
            self.calls.append(("bias_relu_pool2", tuple(z.shape), None, False))
            if plane is not None:
                z = z + scale.reshape(-1, 1, 1, 1) * plane
            if bias is not None:
                z = z + bias.reshape(1, -1, 1, 1)
            return F.max_pool2d(torch.relu(z), 2)

        def pool(x, w, bias, pad):
            self.calls.append(("conv3x3_pool", tuple(x.shape), None, False))
            return block(x, w, bias, pad)

        def pool_planes(x, xp, w, bias, pad, want_planes=False):
            if xp is not None:
                assert self.made[int(xp)] is x, "the planes are not this input's"
            self.calls.append(("conv3x3_pool_planes", tuple(x.shape), int(xp) if xp is not None else None, bool(want_planes)))
            y = block(x, w, bias, pad)
            return (y, token(y)) if want_planes else y

        def first_block(obs, state, w, bias, want_planes=False):
            self.calls.append(("first_block", tuple(obs.shape), None, bool(want_planes)))
            c = obs.shape[1]
            z = F.conv2d(obs, w[:, :c], None, padding=1)
            z = z + state.reshape(-1, 1, 1, 1) * F.conv2d(torch.ones_like(obs[:1, :1]), w[:, c:c + 1], None, padding=1)
            y = F.max_pool2d(torch.relu(z + bias.reshape(1, -1, 1, 1)), 2)
            return (y, token(y)) if want_planes else y

        for n, f in (("conv3x3", conv3x3), ("conv3x3_planes", conv3x3_planes), ("bias_relu_pool2", brp), ("conv3x3_pool", pool),
                     ("conv3x3_pool_planes", pool_planes), ("first_block", first_block)):
            monkeypatch.setattr(H, n, f)

    def names(self):
        return [c[0] for c in self.calls]


def _obs(size, batch):
    g = torch.Generator().manual_seed(size)
    return torch.randn(batch, 1, size, size, generator=g).as_subclass(_OnGpu)


# The size rule below passes the layers the library's thresholds pass at the benchmark's batch and no others: the 3 x 3 -> 1 x 1
# convolutions (and the 128 encoder's 256 -> 256 block) stay with torch's modules, which the recorder does not see.
# the switch off: K10, then conv3x3 + bias_relu_pool2 per pooled block, conv3x3 for the 128 -> 256 layer, K9 alone behind the 256 -> 256 one
TODAY = {84: ["first_block"] + ["conv3x3", "bias_relu_pool2"] * 3 + ["conv3x3"],
         128: ["first_block"] + ["conv3x3", "bias_relu_pool2"] * 3 + ["conv3x3", "bias_relu_pool2"]}
# the switch on: K10 -> K11p x 3 -> K11, each on its predecessor's planes and every one but the last writing its own; then today's calls
CHAIN = ["first_block"] + ["conv3x3_pool_planes"] * 3 + ["conv3x3_planes"]
TAIL = {84: [], 128: ["bias_relu_pool2"]}


@pytest.mark.parametrize("size", [84, 128])
@pytest.mark.parametrize("env", [None, "0", "1"])
def test_base_encoder_carries_planes_only_with_the_switch(size, env, monkeypatch):
    mod = _fresh(env, monkeypatch)
    assert mod.base_encoder.fused_planes == (env == "1") and mod.base_encoder.fused_block is False
    torch.manual_seed(0)
    enc = mod.base_encoder((2, size, size), out_dim=128)
    rec = _Recorder(monkeypatch)
    # the size rule as the library has it, scaled to a batch of 2: the chain's layers pass, the 3 x 3 -> 1 x 1 layers behind it do not
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 1 << 40)
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 2 * 9 if size == 84 else 2 * 64)
    obs, state = _obs(size, 2), torch.tensor([1.0, 0.0])
    with torch.no_grad():
        out = enc.forward_split(obs, state)
        ref = enc.conv(torch.cat([obs.as_subclass(torch.Tensor), state.reshape(-1, 1, 1, 1).expand(-1, 1, size, size)], 1))
    assert torch.allclose(out.as_subclass(torch.Tensor), ref, rtol=1e-4, atol=1e-5)
    if env != "1":
        assert rec.names() == TODAY[size] and not rec.made
        assert all(c[2] is None and c[3] is False for c in rec.calls)
        return
    assert rec.names() == CHAIN + TAIL[size]
    chain = rec.calls[:5]
    assert [c[3] for c in chain] == [True, True, True, True, False]          # every block but the last writes planes
    assert [c[2] for c in chain] == [None, 0, 1, 2, 3]                       # ... and each consumer reads its predecessor's
    assert [c[1][1] for c in chain[1:]] == [16, 32, 64, 128]
    assert all(c[2] is None and c[3] is False for c in rec.calls[5:])
    # a block whose input has no planes runs as today: the un-split forward (the first convolution is the library's, no K10) starts the
    # chain at the 16 -> 32 block, which reads fp32 and writes planes
    rec.calls.clear()
    with torch.no_grad():
        enc(torch.randn(2, 2, size, size).as_subclass(_OnGpu))
    assert rec.names()[:2] == ["bias_relu_pool2", "conv3x3_pool_planes"] and rec.calls[1][2:] == (None, True)
    assert rec.names()[2:5] == ["conv3x3_pool_planes"] * 2 + ["conv3x3_planes"]
    # without K11 there is no K11x
    rec.calls.clear()
    enc.fused_conv = False
    with torch.no_grad():
        enc.forward_split(obs, state)
    assert set(rec.names()) == {"first_block", "bias_relu_pool2"} and not any(c[3] for c in rec.calls)


def test_the_planes_switch_leaves_the_pool_switch_alone(monkeypatch):
    mod = _fresh(None, monkeypatch, pool_env="1")
    assert mod.base_encoder.fused_block is True and mod.base_encoder.fused_planes is False
    mod = _fresh("1", monkeypatch, pool_env="1")
    assert mod.base_encoder.fused_block is True and mod.base_encoder.fused_planes is True


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
