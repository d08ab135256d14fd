"""CPU: the host layer of the narrow gradient builds K11n / K12n (csrc/conv_narrow.hip; aurppo_conv3x3_dgrad_narrow_f32,
aurppo_conv3x3_wgrad_narrow_f32 and their byte queries).  (1) The four symbols are declared, exported and bound.  (2) The byte queries:
0 outside the shape class, the slice plan of tests/narrow_cases.py inside it.  (3) Every refusal carries the entry's name, comes
without a device and so before any HIP call.  (4) What ``hip_ops`` hands to the library with AURPPO_NARROW_GRADS=1 equals
tests/transcripts/conv_narrow_calls.json (the recorder of tests/test_hip_ops_calls.py, imported); unset, the calls are today's.

Re-record with ``python tests/test_conv_narrow_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import narrow_cases as NC                   # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "conv_narrow_calls.json")
EINVAL, ESHAPE = -1, -2
PROTOTYPES = (
    "size_t aurppo_conv3x3_dgrad_narrow_wop_bytes(int Ci, int Co);",
    "int aurppo_conv3x3_dgrad_narrow_f32(const float* dy, const float* w, float* dx, int B, int Ci, int Co, int H, int W, int pad, "
    "void* wop_ws, void* stream);",
    "size_t aurppo_conv3x3_wgrad_narrow_ws_bytes(int B, int Ci, int Co, int H, int W, int pad);",
    "int aurppo_conv3x3_wgrad_narrow_f32(const float* dy, const float* x, float* dw, int B, int Ci, int Co, int H, int W, int pad, "
    "void* ws, void* stream);",
)
NAMES = [re.search(r"(aurppo_\w+)\(", p).group(1) for p in PROTOTYPES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return TC._lib.load()


# ------------------------------------------------------------------ (1) the binding
def test_the_header_declares_the_prototypes_and_the_binding_carries_them(lib):
    with open(os.path.join(ROOT, "include", "aurppo.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for proto, name in zip(PROTOTYPES, NAMES):
        assert proto in header, name
        assert name in TC._lib.SYMBOLS and hasattr(lib, name)
    assert "src/nets/base_cnns.py:32-33" in header
    for name in (NAMES[0], NAMES[2]):
        assert getattr(lib, name).restype is C.c_size_t
    assert list(lib.aurppo_conv3x3_dgrad_narrow_wop_bytes.argtypes) == [C.c_int32] * 2
    assert list(lib.aurppo_conv3x3_wgrad_narrow_ws_bytes.argtypes) == [C.c_int32] * 6
    for name in (NAMES[1], NAMES[3]):
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 2
        assert fn.restype in (C.c_int, C.c_int32)


# ------------------------------------------------------------------ (2) the byte queries
def test_byte_queries_are_zero_outside_the_class(lib):
    dq, wq = lib.aurppo_conv3x3_dgrad_narrow_wop_bytes, lib.aurppo_conv3x3_wgrad_narrow_ws_bytes
    for ci, co in ((17, 32), (0, 32), (16, 48), (16, 0), (16, 16), (16, -32)):
        assert dq(ci, co) == 0, (ci, co)
    for ci in (1, 5, 16):
        for co in (32, 64, 96):
            assert dq(ci, co) == (co // 32) * 27648
    for s in ((2, 17, 32, 8, 8, 1), (2, 16, 33, 8, 8, 1), (2, 16, 32, 8, 8, 3), (2, 16, 32, 8, 8, -1), (2, 16, 32, 2, 8, 0),
              (2, 16, 32, 8, 1, 0), (0, 16, 32, 8, 8, 1), (2, 0, 32, 8, 8, 1), (2, 16, 0, 8, 8, 1)):
        assert wq(*s) == 0, s
    # an image of a gigabyte cannot be addressed from its slice's base: refused, never wrapped
    assert wq(2, 16, 32, 4096, 4096, 1) == 0
    assert wq(1, 1, 1, 1, 1, 1) == 36 and wq(2, 16, 32, 8, 8, 1) == 32 * 16 * 36


@pytest.mark.parametrize("s", NC.WGRAD_SHAPES + [NC.CONFIG3], ids=lambda s: "x".join(map(str, s)))
def test_the_slice_plan_is_what_the_shape_list_says(lib, s):
    plan = NC.wgrad_plan(*s)
    nbytes = lib.aurppo_conv3x3_wgrad_narrow_ws_bytes(*s)
    assert NC.wgrad_slices_from_ws(nbytes, s[1], s[2]) == plan["S"]
    if s in NC.WGRAD_CLAIMS:
        assert (plan["S"], plan["pps"], plan["last"], plan["chunks"], plan["chunks_last"]) == NC.WGRAD_CLAIMS[s]
    else:       # config 3's minibatch: 2048 one-wave slices of 512 chunks, four images each
        assert (plan["S"], plan["pps"], plan["last"], plan["chunks"]) == (2048, 16384, 16384, 512)


def test_every_shape_of_the_list_has_a_claim_and_the_dgrad_plans_hold():
    assert sorted(NC.WGRAD_CLAIMS) == sorted(NC.WGRAD_SHAPES)
    assert NC.dgrad_plan(*NC.DGRAD_SHAPES[0])["tiles"] == 1
    assert NC.dgrad_plan(1, 16, 32, 1, 257, 1)["tiles_x"] == 17
    assert NC.dgrad_plan(3, 16, 64, 10, 10, 1) == dict(tiles_y=2, tiles_x=1, tiles=6, grid=6, groups=2, wop_bytes=2 * 27648)
    assert NC.dgrad_plan(3, 16, 32, 42, 42, 1)["tiles"] == 3 * 6 * 3
    p = NC.dgrad_plan(2100, 3, 32, 2, 2, 1)
    assert p["tiles"] == 2100 and p["grid"] == 2048
    assert NC.dgrad_plan(*NC.CONFIG3)["tiles"] == 8192 * 32


# ------------------------------------------------------------------ (3) refusals: no device, no HIP call
def _err(lib):
    return lib.aurppo_last_error().decode()


def test_refusals_name_their_entry_and_need_no_device(lib):
    p, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)      # never dereferenced: every case below is refused on the host
    dg, wg = lib.aurppo_conv3x3_dgrad_narrow_f32, lib.aurppo_conv3x3_wgrad_narrow_f32
    ok = (2, 16, 32, 8, 8, 1)
    for fn, name in ((dg, NAMES[1]), (wg, NAMES[3])):
        for nulls in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
            assert fn(nulls[0], nulls[1], nulls[2], *ok, nulls[3], None) == EINVAL
            assert name in _err(lib) and "null" in _err(lib)
        assert fn(p, p, p, *ok, odd, None) == EINVAL
        assert name in _err(lib) and "aligned" in _err(lib)
        for bad in ((2, 17, 32, 8, 8, 1), (2, 0, 32, 8, 8, 1), (2, 16, 32, 8, 8, 3), (2, 16, 32, 8, 8, -1), (0, 16, 32, 8, 8, 1),
                    (2, 16, 32, 0, 8, 1), (2, 16, 32, 2, 8, 0), (2, 16, 32, 8, 1, 0)):
            assert fn(p, p, p, *bad, p, None) == ESHAPE, bad
            assert name in _err(lib)
    assert dg(p, p, p, 2, 16, 48, 8, 8, 1, p, None) == ESHAPE and NAMES[1] in _err(lib)
    assert wg(p, p, p, 2, 16, 33, 8, 8, 1, p, None) == ESHAPE and NAMES[3] in _err(lib)
    assert wg(p, p, p, 2, 16, 32, 4096, 4096, 1, p, None) == ESHAPE and NAMES[3] in _err(lib)
    assert dg(p, p, p, 2, 16, 32, 46341, 46341, 1, p, None) == ESHAPE and NAMES[1] in _err(lib)


def test_an_accepted_call_without_a_device_fails_in_hip_not_before(lib):
    """The other half of "refusals precede every HIP call": what is not refused reaches the runtime, which has no device here."""
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a device")
    p = C.c_void_p(0x1000)
    assert lib.aurppo_conv3x3_wgrad_narrow_f32(p, p, p, 2, 16, 32, 8, 8, 1, p, None) == -3
    assert lib.aurppo_conv3x3_dgrad_narrow_f32(p, p, p, 2, 16, 32, 8, 8, 1, p, None) == -3


# ------------------------------------------------------------------ (4) routing, through the recording stand-in
def _narrow_ok_without_a_device(t):
    """``hip_ops._narrow_tensor_ok`` with ``is_cuda`` dropped, as the recorder's ``_ptr`` drops it: the recorder's tensors live on the CPU."""
    return t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()


def _backward_case(h):
    x, w = h.t("x", 2, 16, 4, 5).requires_grad_(True), h.t("w", 32, 16, 3, 3).requires_grad_(True)
    z = H.conv3x3(x, w, 1)
    h.name("z", z)
    z.backward(h.t("g", 2, 32, 4, 5))
    assert x.grad.shape == x.shape and w.grad.shape == w.shape


CASES = {"conv3x3/backward/narrow": _backward_case}


def run_case(name, setattr_, setenv, bound=None):
    h = TC.Harness(bound)
    h.install(setattr_)
    setattr_(H, "_narrow_tensor_ok", _narrow_ok_without_a_device)
    setattr_(H, "NARROW_MIN_PIXELS", 1)
    setenv("AURPPO_NARROW_GRADS", "1")
    # (autograd hands a leaf its own copy of a gradient: the tensors the two functions allocate are named where they are returned)
    real_d, real_w = H.conv3x3_dgrad_narrow, H.conv3x3_wgrad_narrow
    setattr_(H, "conv3x3_dgrad_narrow", lambda g, w, pad: h.name("dx", real_d(g, w, pad)))
    setattr_(H, "conv3x3_wgrad_narrow", lambda g, x, cout, pad: h.name("dw", real_w(g, x, cout, pad)))
    CASES[name](h)
    return json.loads(json.dumps(h.transcript()))


def _recorded():
    with open(TRANSCRIPT) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(_recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_match_the_recorded_transcript(name, monkeypatch):
    got, want = run_case(name, monkeypatch.setattr, monkeypatch.setenv), _recorded()[name]
    assert len(got) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs"
    assert len(got) == len(want)


def test_the_two_narrow_calls_carry_every_pointer_in_its_declared_place(monkeypatch, lib):
    calls = run_case("conv3x3/backward/narrow", monkeypatch.setattr, monkeypatch.setenv, lib)
    names = [c[0] for c in calls]
    assert names == ["aurppo_conv3x3_wop_bytes", "_workspace", "aurppo_conv3x3_f32",
                     "aurppo_conv3x3_dgrad_narrow_wop_bytes", "aurppo_conv3x3_dgrad_narrow_wop_bytes", "_workspace", "aurppo_conv3x3_dgrad_narrow_f32",
                     "aurppo_conv3x3_wgrad_narrow_ws_bytes", "aurppo_conv3x3_wgrad_narrow_ws_bytes", "_workspace", "aurppo_conv3x3_wgrad_narrow_f32"]
    by = {c[0]: c[1] for c in calls}
    #                                                 dy     w / x   dx / dw  B  Ci  Co  H  W  pad  workspace            stream
    assert by["aurppo_conv3x3_dgrad_narrow_f32"] == ["g+0", "w+0", "dx+0", 2, 16, 32, 4, 5, 1, "ws:dgrad_narrow+0", "stream"]
    assert by["aurppo_conv3x3_wgrad_narrow_f32"] == ["g+0", "x+0", "dw+0", 2, 16, 32, 4, 5, 1, "ws:wgrad_narrow+0", "stream"]
    assert by["aurppo_conv3x3_dgrad_narrow_wop_bytes"] == [16, 32] and by["aurppo_conv3x3_wgrad_narrow_ws_bytes"] == [2, 16, 32, 4, 5, 1]
    assert [c[1][0] for c in calls if c[0] == "_workspace"] == ["conv", "dgrad_narrow", "wgrad_narrow"]


def _today(monkeypatch, env, lift):
    h = TC.Harness()
    with monkeypatch.context() as m:
        h.install(m.setattr)
        m.setattr(H, "_narrow_tensor_ok", _narrow_ok_without_a_device)
        if lift:
            m.setattr(H, "NARROW_MIN_PIXELS", 1)
        if env is None:
            m.delenv("AURPPO_NARROW_GRADS", raising=False)
        else:
            m.setenv("AURPPO_NARROW_GRADS", env)
        _backward_case(h)
    return [c[0] for c in h.calls]


def test_unset_or_under_the_size_rule_the_calls_are_todays(monkeypatch):
    """Today: the forward's three calls, both gradients from the library (aten, which the recorder does not see).  The same with the
    switch at "0", and with it set while the size rule holds (40 pixels)."""
    today = ["aurppo_conv3x3_wop_bytes", "_workspace", "aurppo_conv3x3_f32"]
    assert _today(monkeypatch, None, True) == today
    assert _today(monkeypatch, "0", True) == today
    assert H.NARROW_MIN_PIXELS > 40
    got = _today(monkeypatch, "1", False)
    assert [n for n in got if "narrow_f32" in n] == [] and [n for n in got if "narrow" not in n] == today
    # ... and the recorded transcript of today's route (tests/transcripts/hip_ops_calls.json) is made with the variable unset
    monkeypatch.delenv("AURPPO_NARROW_GRADS", raising=False)
    with open(TC.TRANSCRIPT) as f:
        want = json.load(f)["conv3x3/dx_aten"]
    h = TC.Harness()
    with monkeypatch.context() as m:
        h.install(m.setattr)
        TC.CASES["conv3x3/dx_aten"](h)
    assert json.loads(json.dumps(h.transcript())) == want


def test_the_predicates(monkeypatch):
    import types
    monkeypatch.setattr(H, "_lib_or_raise", lambda: TC._lib.load())

    def like(*shape, dtype=torch.float32, cuda=True, contiguous=True):
        return types.SimpleNamespace(shape=tuple(shape), dtype=dtype, is_cuda=cuda, dim=lambda: len(shape), is_contiguous=lambda: contiguous)
    g, x, w = like(8192, 32, 64, 64), like(8192, 16, 64, 64), like(32, 16, 3, 3)
    assert H.conv3x3_dgrad_narrow_ok(g, w, 1) and H.conv3x3_wgrad_narrow_ok(g, x, 32, 1)
    assert not H.conv3x3_dgrad_narrow_ok(like(8, 32, 64, 64), w, 1) and not H.conv3x3_wgrad_narrow_ok(like(8, 32, 64, 64), like(8, 16, 64, 64), 32, 1)
    monkeypatch.setattr(H, "NARROW_MIN_PIXELS", 1)
    assert H.conv3x3_dgrad_narrow_ok(like(8, 32, 64, 64), w, 1) and H.conv3x3_wgrad_narrow_ok(like(8, 32, 64, 64), like(8, 16, 64, 64), 32, 1)
    for bad in (like(8192, 32, 64, 64, cuda=False), like(8192, 32, 64, 64, dtype=torch.float64), like(8192, 32, 64, 64, contiguous=False),
                like(8192 * 32, 64, 64)):
        assert not H.conv3x3_dgrad_narrow_ok(bad, w, 1) and not H.conv3x3_wgrad_narrow_ok(bad, x, 32, 1)
    assert not H.conv3x3_dgrad_narrow_ok(g, like(32, 17, 3, 3), 1) and not H.conv3x3_dgrad_narrow_ok(like(8192, 48, 64, 64), like(48, 16, 3, 3), 1)
    assert not H.conv3x3_dgrad_narrow_ok(g, w, 3) and not H.conv3x3_wgrad_narrow_ok(g, x, 32, 3)
    assert not H.conv3x3_wgrad_narrow_ok(like(8192, 33, 64, 64), x, 33, 1) and not H.conv3x3_wgrad_narrow_ok(g, like(8192, 17, 64, 64), 32, 1)
    assert not H.conv3x3_wgrad_narrow_ok(g, x, 32, 0)          # dy's map is not the one pad 0 gives


if __name__ == "__main__":
    class _Patch:
        def __init__(self):
            self.undo, self.env = [], []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

        def setenv(self, name, value):
            self.env.append((name, os.environ.get(name)))
            os.environ[name] = value

        def restore(self):
            for obj, name, old in reversed(self.undo):
                setattr(obj, name, old)
            for name, old in reversed(self.env):
                if old is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = old

    result = {}
    for case_name in sorted(CASES):
        patch = _Patch()
        try:
            result[case_name] = run_case(case_name, patch.setattr, patch.setenv)
        finally:
            patch.restore()
    os.makedirs(os.path.dirname(TRANSCRIPT), exist_ok=True)
    with open(TRANSCRIPT, "w") as f:
        f.write(TC._dump(result))
    print(f"{len(result)} cases, {sum(len(v) for v in result.values())} calls -> {TRANSCRIPT}")
