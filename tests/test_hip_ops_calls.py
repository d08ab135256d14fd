"""CPU: what ``aur_ppo_amd.hip_ops`` hands to the C ABI -- every library call and workspace request of every entry point, in
order, with every pointer resolved to the tensor (and byte offset) it points into -- equals the recorded transcript
tests/transcripts/hip_ops_calls.json.  The argument lists of include/aurppo.h are rows of same-typed pointers: a transposition
raises nothing on the host and faults on the GPU, so the order is pinned here, without a GPU and without the library.

Seams replaced: ``hip_ops._lib_or_raise`` / ``_lib.load`` (a recorder that returns 0; ``*_bytes`` / ``*_parts`` return a fixed
arithmetic function of their arguments), ``hip_ops._ptr`` (dtype and contiguity checks kept, ``is_cuda`` dropped; it keeps every
tensor it sees alive, so no address is reused within a case), ``hip_ops._stream``, ``hip_ops._workspace`` (records (kind, nbytes),
hands back a named CPU byte tensor).  Two cases need one more stand-in, in torch and not in the layer under test: MT19937 and P2PExchange enter
``torch.cuda.device`` with the device they are given (torch accepts only a GPU there: a null context), and the layered step keys its
activation buffers by ``torch.cuda.current_device()`` when the tensors' device has no index (0).

Re-record (``python tests/test_hip_ops_calls.py``) and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from aur_ppo_amd import _lib, hip_ops as H                     # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic              # noqa: E402
from aur_ppo_amd.flat import FlatBucket                        # noqa: E402

TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "hip_ops_calls.json")
STREAM, EV0, EV1 = 0x57000, 0xE0100, 0xE0200
M, B, A = 5, 7, 3
CLIP, ENT, VF, MAX_NORM, BETAS, EPS = 0.2, 0.01, 0.5, 0.7, (0.9, 0.95), 1e-5


class _Lib:
    def __init__(self, h, bound=None):
        self._h, self._bound = h, bound

    def __getattr__(self, fn):
        if fn.startswith("_"):
            raise AttributeError(fn)

        def call(*args):
            if self._bound is not None:         # the real binding: as many arguments as argtypes, each one convertible
                argtypes = getattr(self._bound, fn).argtypes or ()
                assert len(args) == len(argtypes), f"{fn}: {len(args)} arguments passed, {len(argtypes)} bound"
                for t, a in zip(argtypes, args):
                    t.from_param(a)
            self._h.calls.append([fn, [self._h.raw(a) for a in args]])
            if fn.endswith(("_bytes", "_parts")):
                return 64 + 16 * sum((i + 1) * int(a) for i, a in enumerate(args))
            return 0
        return call


class Harness:
    def __init__(self, bound=None):
        self.calls, self.named, self.keep, self.ws = [], [], [], {}
        self.consts = {STREAM: "stream", EV0: "ev0", EV1: "ev1"}
        self.lib = _Lib(self, bound)

    def install(self, setattr_):
        setattr_(H, "_lib_or_raise", lambda: self.lib)
        setattr_(_lib, "load", lambda: self.lib)
        setattr_(H, "_ptr", self._ptr)
        setattr_(H, "_stream", lambda: C.c_void_p(STREAM))
        setattr_(H, "_workspace", self._workspace)

    # ---- the seams
    def _ptr(self, t, dtype=torch.float32):
        if not (t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"expected a contiguous {dtype} tensor, got {t.dtype}, contiguous={t.is_contiguous()}")
        self.keep.append(t)
        return C.c_void_p(t.data_ptr())

    def _workspace(self, kind, nbytes, device):
        self.calls.append(["_workspace", [kind, int(nbytes)]])
        ws = self.ws.get(kind)
        if ws is None or ws.numel() < nbytes:
            ws = self.ws[kind] = self.name(f"ws:{kind}", torch.zeros(nbytes, dtype=torch.uint8))
        return ws

    # ---- named tensors
    def name(self, name, t):
        self.named.append((name, t.data_ptr(), t.data_ptr() + max(1, t.numel() * t.element_size())))
        self.keep.append(t)
        return t

    def t(self, name, *shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        return self.name(name, ((torch.arange(n) % 7 - 3).to(torch.float32) * 0.25).to(dtype).reshape(shape).contiguous())

    def idx(self, name, n=M):
        return self.name(name, (torch.arange(n, dtype=torch.int32) * 3 % B).contiguous())

    # ---- normalisation: raw while recording, names once the case has named what the call returned
    def raw(self, a):
        if a is None:
            return None
        if isinstance(a, C.c_void_p):
            return ("p", a.value) if a.value else None
        if isinstance(a, C.Array):
            if a._type_ is C.c_char:
                return ["chars", len(a)]
            return [(("p", x) if x else None) if a._type_ is C.c_void_p else self.raw(x) for x in a]
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, int):
            return ("i", a)
        if isinstance(a, float):
            return a
        if isinstance(a, C._SimpleCData):
            return self.raw(a.value)
        return type(a).__name__           # byref(...) / POINTER(...) of a host object

    def _resolve(self, v):
        if isinstance(v, list):
            return [self._resolve(x) for x in v]
        if not isinstance(v, tuple):
            return v
        kind, x = v
        if x in self.consts:
            return self.consts[x]
        for name, lo, hi in self.named:
            if lo <= x < hi:
                return f"{name}+{x - lo}"
        return "anon" if kind == "p" else x

    def transcript(self):
        return [[fn, self._resolve(args)] for fn, args in self.calls]


class _Events:
    def __init__(self, handle):
        self.cuda_event, self.recorded = handle, 0

    def record(self):
        self.recorded += 1


# ------------------------------------------------------------------ the cases
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def _policy(h, D, Hd, NL, cont):
    pol = actor_critic(D, (A,) if cont else A, Hd, NL, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    h.name("param", bucket.flat_param)
    h.name("grad", bucket.flat_grad)
    return pol, bucket


def _mlp(h, kind, cont=True, packed=False):
    """(layout, bucket, obs, actions, rec, idx) of a narrow (2 x 64, D 8), wide (3 x 96, D 8) or layered (hand-built: 128, D 16) policy."""
    D, Hd, NL = {"narrow": (8, 64, 2), "wide": (8, 96, 3), "layered1": (16, 128, 1), "layered3": (16, 128, 3)}[kind]
    pol, bucket = _policy(h, D, Hd, NL, cont)
    if kind.startswith("layered"):
        seq, pos, D_, A_, cont_, NL_, Hd_ = H._mlp_structure(pol, bucket)
        lay = dict(offsets=seq, n_params=pos, D=D_, A=A_, continuous=cont_, hidden=Hd_, num_layers=NL_, layered=True)
    else:
        lay = H.mlp_layout(pol, bucket)
        assert lay is not None and bool(lay.get("wide")) == (kind == "wide")
    assert lay["offsets"][2] != 0 and lay["continuous"] == cont
    obs = h.t("obs", B, D)
    if packed:
        actions, rec = None, h.t("rec64", B, 16)
    else:
        actions, rec = (h.t("actions", B, A) if cont else h.t("actions", B)), h.t("rec", B, 4)
    return lay, bucket, obs, actions, rec, h.idx("idx")


def _adam(h, bucket):
    return (h.name("exp_avg", torch.zeros_like(bucket.flat_param)), h.name("exp_avg_sq", torch.zeros_like(bucket.flat_param)),
            h.t("lr", 1), h.t("step", 1), h.t("norms", 4))


@case("gae")
def _(h):
    T, N = 3, 2
    r, v, d, lp = h.t("rewards", T, N), h.t("values", T, N), h.t("terminals", T, N), h.t("log_probs", T, N)
    nv, nd = h.t("next_value", N), h.t("next_done", N)
    ret, adv = H.gae(r, v, d, nv, nd, 0.99, 0.95, H.NORMAL_ADV)
    h.name("ret", ret), h.name("adv", adv)
    out = (h.t("ret2", T, N), h.t("adv2", T, N))
    assert H.gae(r, v, d, nv, nd, 0.98, 0.9, H.GAE_SKIP_LAST, out=out, log_probs=lp, rec=h.t("rec", T * N, 4))[0] is out[0]


@case("mt19937")
def _(h):
    rng = H.MT19937(2 ** 32 + 7, 16, device="cpu")
    rng.seed(11)
    key, pos = rng.get_state()
    rng.set_state(key, 3)
    rng.status_into(h.t("flag", 1))
    rng.shuffle_(h.idx("idx", 6))
    rng.shuffle_(torch.empty(0, dtype=torch.int32))
    rng.shuffle_epochs(6, 2, out=h.name("perms", torch.zeros((2, 6), dtype=torch.int32)))
    h.name("perms2", rng.shuffle_epochs(4, 3))


@case("arange_i32")
def _(h):
    h.name("out", H.arange_i32(6, "cpu"))


@case("gather")
def _(h):
    srcs = [h.t("obs", B, 8), h.t("actions", B, 3), h.t("rec", B, 4)]
    for i, o in enumerate(H.gather(h.idx("idx"), srcs)):
        h.name(f"out{i}", o)
    outs = [h.t("o_obs", M, 8), h.t("o_actions", M, 3), h.t("o_rec", M, 4)]
    H.gather(h.idx("idx2"), srcs, outs)


def _loss_inputs(h):
    return {k: h.t(k, *((M, 1) if k == "newv" else (M,))) for k in ("newlogp", "oldlogp", "adv", "newv", "oldv", "ret", "entropy")}


@case("loss_fwd_bwd")
def _(h):
    t = _loss_inputs(h)
    out = H.loss_fwd_bwd(t["newlogp"], t["oldlogp"], t["adv"], t["newv"], t["oldv"], t["ret"], t["entropy"], CLIP, ENT, VF,
                         norm_adv=False, vloss_mode=H.VLOSS_OLDVALUES)
    for n, o in zip(("scalars", "g_lp", "g_v", "g_e"), out):
        h.name(n, o)
    H.loss_fwd_bwd(t["newlogp"], t["oldlogp"], t["adv"], t["newv"], t["oldv"], t["ret"], t["entropy"], CLIP, ENT, VF,
                   out_scalars=h.t("scalars2", 9))


@case("loss_fwd_bwd_packed")
def _(h):
    t = _loss_inputs(h)
    out = H.loss_fwd_bwd_packed(t["newlogp"], t["newv"], t["entropy"], h.t("rec", M, 4), CLIP, ENT, VF, norm_adv=False,
                                vloss_mode=H.VLOSS_RETURNS, out_scalars=h.t("scalars", 9))
    for n, o in zip(("scalars", "g_lp", "g_v", "g_e"), out):
        h.name(n, o)


def _loss_autograd(h, packed):
    t = _loss_inputs(h)
    for k in ("newlogp", "newv", "entropy"):
        t[k].requires_grad_(True)
    sc = h.t("scalars", 9)
    if packed:
        loss = H.ppo_loss_packed(t["newlogp"], t["newv"], t["entropy"], h.t("rec", M, 4), CLIP, ENT, VF, True, H.VLOSS_CLIPPED, sc)
    else:
        loss = H.ppo_loss(t["newlogp"], t["newv"], t["entropy"], t["oldlogp"], t["adv"], t["oldv"], t["ret"], CLIP, ENT, VF, True,
                          H.VLOSS_CLIPPED, sc)
    (2.0 * loss).backward()
    assert t["newv"].grad.shape == (M, 1) and t["newlogp"].grad.shape == (M,) and t["entropy"].grad.shape == (M,)
    assert loss.shape == () and loss.data_ptr() != sc.data_ptr()


@case("ppo_loss")
def _(h):
    _loss_autograd(h, False)


@case("ppo_loss_packed")
def _(h):
    _loss_autograd(h, True)


@case("pack_records")
def _(h):
    h.name("out", H.pack_records(h.t("rec", B, 4), h.t("actions", B, A)))
    H.pack_records(h.t("rec2", B, 4), h.t("actions1", B), out=h.t("rec64", B, 16))


def _step_case(kind, cont, packed, events):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _mlp(h, kind, cont, packed)
        ev = (_Events(EV0), _Events(EV1)) if events else None
        sc = h.t("scalars", 9) if events else None
        out = H.mlp_ppo_step(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, norm_adv=not events,
                             vloss_mode=H.VLOSS_OLDVALUES, out_scalars=sc, events=ev)
        assert (out is sc) if events else out.shape == (9,)
        assert ev is None or (ev[0].recorded, ev[1].recorded) == (1, 1)
        h.name("scalars_new", out)
    return run


for _kind in ("narrow", "wide"):
    for _cont in (True, False):
        for _packed in (False, True):
            for _events in (False, True):
                CASES[f"mlp_ppo_step/{_kind}/{'continuous' if _cont else 'categorical'}/{'packed' if _packed else 'separate'}/"
                      f"{'events' if _events else 'plain'}"] = _step_case(_kind, _cont, _packed, _events)


def _minibatch_case(kind, with_next, chained):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _mlp(h, kind, True, True)
        m, v, lr, step, norms = _adam(h, bucket)
        sc = h.t("scalars", 2, 9)
        out = H.mlp_ppo_minibatch(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, True, H.VLOSS_CLIPPED,
                                  sc[1], m, v, lr, step, MAX_NORM, BETAS, EPS, norms[1:2], next_idx=h.idx("next_idx", M - 1) if with_next else None,
                                  chained=chained)
        assert out.data_ptr() == sc[1].data_ptr()
    return run


for _kind in ("narrow", "wide"):
    for _next in (False, True):
        for _chained in (False, True):
            CASES[f"mlp_ppo_minibatch/{_kind}/{'next' if _next else 'last'}/{'chained' if _chained else 'first'}"] = \
                _minibatch_case(_kind, _next, _chained)


@case("mlp_ppo_grad")
def _(h):
    lay, bucket, obs, actions, rec, idx = _mlp(h, "narrow", False, False)
    H.mlp_ppo_grad(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, False, H.VLOSS_RETURNS, h.t("scalars", 9),
                   h.t("step", 1))
    H.mlp_ppo_grad(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, True, H.VLOSS_CLIPPED, h.t("scalars2", 9),
                   h.t("step2", 1), chained=True)


def _apply_case(parts):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _mlp(h, "narrow", True, True)
        m, v, lr, step, norms = _adam(h, bucket)
        extra = (h.name("sq_part", torch.zeros(6, dtype=torch.float64)),) if parts else ()
        fn = H.mlp_ppo_apply_parts if parts else H.mlp_ppo_apply
        assert fn(bucket.flat_param, bucket.flat_grad, m, v, lay, lr, step, MAX_NORM, BETAS, EPS, norms[0:1], *extra).data_ptr() == norms.data_ptr()
        kw = {} if parts else {"grad_scale": 0.25}
        fn(bucket.flat_param, bucket.flat_grad, m, v, lay, lr, step, MAX_NORM, BETAS, EPS, norms[2:3], *extra, rec=rec,
           next_idx=h.idx("next_idx", M - 1), **kw)
        fn(bucket.flat_param, bucket.flat_grad, m, v, lay, lr, step, MAX_NORM, BETAS, EPS, norms[3:4], *extra, rec=h.t("rec4", B, 4), **kw)
    return run


CASES["mlp_ppo_apply"] = _apply_case(False)
CASES["mlp_ppo_apply_parts"] = _apply_case(True)


def _act_case(kind, cont, noise):
    def run(h):
        N = 4
        lay, bucket, *_ = _mlp(h, kind, cont, False)
        obs = h.t("obs4", N, lay["D"])
        if not noise:
            a, lp, v = H.mlp_act(obs, None, bucket.flat_param, lay)
            assert a is None and lp is None
            h.name("value_new", v)
            H.mlp_act(obs, None, bucket.flat_param, lay, value=h.t("value", N))
            return
        nz = h.t("noise", N, A) if cont else h.t("noise", N)
        for n, o in zip(("actions_new", "logp_new", "value_new"), H.mlp_act(obs, nz, bucket.flat_param, lay)):
            assert o.shape == ((N, A) if cont and n == "actions_new" else (N,))
            h.name(n, o)
        H.mlp_act(obs, nz, bucket.flat_param, lay, actions=h.t("actions_out", N, A) if cont else h.t("actions_out", N), logp=h.t("logp", N),
                  value=h.t("value", N))
    return run


for _kind in ("narrow", "wide"):
    for _cont in (True, False):
        for _noise in (True, False):
            CASES[f"mlp_act/{_kind}/{'continuous' if _cont else 'categorical'}/{'noise' if _noise else 'value_only'}"] = \
                _act_case(_kind, _cont, _noise)


@case("grad_norm_clip_")
def _(h):
    h.name("norm_new", H.grad_norm_clip_(h.t("grad", 10), MAX_NORM))
    H.grad_norm_clip_(h.t("grad2", 12), MAX_NORM, h.t("norm", 1))


@case("clip_adam_")
def _(h):
    p, g, m, v, lr, step = (h.t(k, n) for k, n in (("param", 12), ("grad", 12), ("exp_avg", 12), ("exp_avg_sq", 12), ("lr", 1), ("step", 1)))
    h.name("norm_new", H.clip_adam_(p, g, m, v, lr, step, MAX_NORM))
    H.clip_adam_(p, g, m, v, lr, step, MAX_NORM, 8, BETAS, EPS, h.t("norm", 1))


@case("bias_relu_pool2")
def _(h):
    Bn, Cc, Hh, Ww = 2, 3, 4, 6
    x, bias = h.t("x", Bn, Cc, Hh, Ww).requires_grad_(True), h.t("bias", Cc).requires_grad_(True)
    scale, plane = h.t("scale", Bn), h.t("plane", 1, Cc, Hh, Ww).requires_grad_(True)
    y = H.bias_relu_pool2(x, bias, scale, plane)
    assert y.shape == (Bn, Cc, Hh // 2, Ww // 2)
    h.name("y", y)
    y.backward(h.t("dy", Bn, Cc, Hh // 2, Ww // 2))
    h.name("dx", x.grad)
    assert bias.grad.shape == (Cc,) and plane.grad.shape == (1, Cc, Hh, Ww)
    x2 = h.t("x2", Bn, Cc, Hh, Ww).requires_grad_(True)
    y2 = H.bias_relu_pool2(x2)
    h.name("y2", y2)
    y2.backward(h.t("dy2", Bn, Cc, Hh // 2, Ww // 2))
    h.name("dx2", x2.grad)


@case("first_block")
def _(h):
    Bn, Ci, Co, Hh, Ww = 2, 3, 16, 4, 6
    w, bias = h.t("weight", Co, Ci + 1, 3, 3).requires_grad_(True), h.t("bias", Co).requires_grad_(True)
    y = H.first_block(h.t("obs", Bn, Ci, Hh, Ww), h.t("state", Bn, 1), w, bias)
    h.name("y", y)
    y.backward(h.t("dy", Bn, Co, Hh // 2, Ww // 2))
    assert w.grad.shape == (Co, Ci + 1, 3, 3) and bias.grad.shape == (Co,)
    w2 = h.t("weight2", Co, Ci + 1, 3, 3).requires_grad_(True)
    y2 = H.first_block(h.t("obs2", Bn, Ci, Hh, Ww), h.t("state2", Bn), w2, None)
    h.name("y2", y2)
    y2.backward(h.t("dy2", Bn, Co, Hh // 2, Ww // 2))


def _conv_case(Ci):
    def run(h):
        Bn, Co, Hh, Ww, pad = 2, 64, 4, 5, 1
        x, w = h.t("x", Bn, Ci, Hh, Ww).requires_grad_(True), h.t("w", Co, Ci, 3, 3).requires_grad_(True)
        z = H.conv3x3(x, w, pad)
        assert z.shape == (Bn, Co, Hh, Ww)
        h.name("z", z)
        z.backward(h.t("g", Bn, Co, Hh, Ww))
        h.name("dx", x.grad)
        assert x.grad.shape == x.shape and w.grad.shape == w.shape
    return run


CASES["conv3x3/dx_library"] = _conv_case(32)
CASES["conv3x3/dx_aten"] = _conv_case(16)


@case("conv3x3_wgrad")
def _(h):
    Bn, Ci, Co, Hh, Ww, pad = 2, 4, 8, 5, 6, 2
    h.name("dw", H.conv3x3_wgrad(h.t("g", Bn, Co, Hh + 2, Ww + 2), h.t("x", Bn, Ci, Hh, Ww), Co, pad))


@case("linear_nobias")
def _(h):
    h.name("y0", H.linear_nobias(h.t("x", M, 16), h.t("w", 32, 16)))
    h.name("y1", H.linear_nobias(h.t("dy", M, 32), h.t("w", 32, 16), mode=1))


@case("linear_bias_act")
def _(h):
    h.name("y0", H.linear_bias_act(h.t("x", M, 16), h.t("w", 32, 16), h.t("bias", 32), act=1))
    h.name("y1", H.linear_bias_act(h.t("x2", M, 16), h.t("w2", 32, 16), None))


@case("linear_rows_bias_act")
def _(h):
    h.name("y0", H.linear_rows_bias_act(h.t("x", B, 16), h.idx("rows"), h.t("w", 32, 16), h.t("bias", 32), act=1))
    h.name("y1", H.linear_rows_bias_act(h.t("x2", B, 16), h.idx("rows2", M - 1), h.t("w2", 32, 16), None))


@case("linear_wgrad")
def _(h):
    h.name("dw", H.linear_wgrad(h.t("gy", M, 32), h.t("x", M, 16)))


@case("linear_wgrad_rows")
def _(h):
    h.name("dw", H.linear_wgrad_rows(h.t("gy", M, 32), h.t("x", B, 16), h.idx("rows")))


@case("linear_dx_tanh")
def _(h):
    gz, w, hh = h.t("gz", M, 32), h.t("w", 32, 16), h.t("h", M, 16)
    h.name("out_new", H.linear_dx_tanh(gz, w, hh))
    assert H.linear_dx_tanh(gz, w, hh, out=hh) is hh


def _head_case(cont, packed):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _mlp(h, "layered3", cont, packed)
        hA, hC = h.t("hA", M, 128), h.t("hC", M, 128)
        h.name("scalars_new", H.head_ppo(hA, hC, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF))
        H.head_ppo(hA, hC, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, False, H.VLOSS_RETURNS,
                   h.t("scalars", 9), gzA=h.t("gzA", M, 128), gzC=h.t("gzC", M, 128))
    return run


CASES["head_ppo/continuous/separate"] = _head_case(True, False)
CASES["head_ppo/categorical/packed"] = _head_case(False, True)


def _layered_case(kind, cont, packed):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _mlp(h, kind, cont, packed)
        H._layered_cache.clear()
        sc = h.t("scalars", 9)
        assert H.mlp_layered_step(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, True, H.VLOSS_OLDVALUES,
                                  sc) is sc
        for net, acts in enumerate(H._layered_buffers(M, lay, obs.device)):
            for l, a in enumerate(acts):
                h.name(f"act{net}.{l}", a)
        H._layered_cache.clear()
    return run


CASES["mlp_layered_step/L1"] = _layered_case("layered1", True, True)
CASES["mlp_layered_step/L3"] = _layered_case("layered3", False, False)


@case("p2p_exchange")
def _(h):
    x = H.P2PExchange(0, 1, 40, "cpu", lambda b: [b])
    h.name("sq_part", x.sq_part)
    x.allreduce_mean_(h.t("grad", 40), 36, h.t("step", 1), timeout_s=2.5)
    assert x.parts(36).numel() == 64 + 16 * 36 and x.status() == 0
    x.close()


# ------------------------------------------------------------------ running, recording, checking
def run_case(name, setattr_, bound=None):
    h = Harness(bound)
    h.install(setattr_)
    if name in ("mt19937", "p2p_exchange"):
        setattr_(torch.cuda, "device", lambda d: contextlib.nullcontext())
    if name.startswith("mlp_layered_step"):
        setattr_(torch.cuda, "current_device", lambda: 0)
    CASES[name](h)
    return json.loads(json.dumps(h.transcript()))


def _recorded():
    with open(TRANSCRIPT) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(_recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_match_the_recorded_transcript(name, monkeypatch):
    if name == "p2p_exchange":
        monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    got, want = run_case(name, monkeypatch.setattr), _recorded()[name]
    assert len(got) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs"
    assert len(got) == len(want)


def test_every_call_fits_the_bound_argtypes(monkeypatch):
    """The same cases against the real binding's ``argtypes`` (count and ctypes conversion; nothing is launched): together with
    tests/test_abi_signatures.py this ties what ``hip_ops`` passes to what include/aurppo.h declares."""
    import __graft_entry__ as g
    g.build()
    bound = _lib.load()
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


def _bad_cases():
    """(entry point, what is wrong) -> a call that must raise ValueError before anything reaches the library."""
    def narrow(h, packed=False):
        return _mlp(h, "narrow", True, packed)

    def step_like(fn, kind, tail=()):
        def run(h, what):
            lay, bucket, obs, actions, rec, idx = _mlp(h, kind, True, False)
            p, g = bucket.flat_param, bucket.flat_grad
            if what == "rec":
                rec = h.t("rec5", B, 5)
            extra = tail(h, bucket) if tail else ()
            if what == "bucket":
                g = h.t("short", lay["n_params"] - 1)
            fn(obs, actions, rec, idx, p, lay, g, CLIP, ENT, VF, True, H.VLOSS_CLIPPED, h.t("scalars", 9), *extra)
        return run

    def mb_tail(h, bucket):
        m, v, lr, step, norms = _adam(h, bucket)
        return (m, v, lr, step, MAX_NORM, BETAS, EPS, norms[0:1])

    def apply_like(fn, parts):
        def run(h, what):
            lay, bucket, *_ = _mlp(h, "wide" if what == "wide" else "narrow", True, False)
            m, v, lr, step, norms = _adam(h, bucket)
            if what == "bucket":
                m = h.t("short", lay["n_params"] - 1)
            extra = (h.name("sq_part", torch.zeros(6, dtype=torch.float64)),) if parts else ()
            fn(bucket.flat_param, bucket.flat_grad, m, v, lay, lr, step, MAX_NORM, BETAS, EPS, norms[0:1], *extra)
        return run

    def head(h, what):
        lay, bucket, obs, actions, rec, idx = _mlp(h, "layered3", True, False)
        g = h.t("short", lay["n_params"] - 1) if what == "bucket" else bucket.flat_grad
        rec = h.t("rec5", B, 5) if what == "rec" else rec
        H.head_ppo(h.t("hA", M, 128), h.t("hC", M, 128), actions, rec, idx, bucket.flat_param, lay, g, CLIP, ENT, VF)

    def layered(h, what):
        lay, bucket, obs, actions, rec, idx = _mlp(h, "layered1", True, False)
        g = h.t("short", lay["n_params"] - 1) if what == "bucket" else bucket.flat_grad
        rec = h.t("rec5", B, 5) if what == "rec" else rec
        H.mlp_layered_step(obs, actions, rec, idx, bucket.flat_param, lay, g, CLIP, ENT, VF)

    def grad(h, what):
        lay, bucket, obs, actions, rec, idx = _mlp(h, "wide" if what == "wide" else "narrow", True, False)
        rec = h.t("rec5", B, 5) if what == "rec" else rec
        H.mlp_ppo_grad(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, CLIP, ENT, VF, True, H.VLOSS_CLIPPED, h.t("scalars", 9),
                       h.t("step", 1))

    out = {}
    for kind in ("narrow", "wide"):
        out[f"mlp_ppo_step/{kind}", "rec"] = step_like(H.mlp_ppo_step, kind)
        out[f"mlp_ppo_minibatch/{kind}", "rec"] = out[f"mlp_ppo_minibatch/{kind}", "bucket"] = step_like(H.mlp_ppo_minibatch, kind, mb_tail)
    out["mlp_ppo_grad", "rec"] = out["mlp_ppo_grad", "wide"] = grad
    out["mlp_ppo_apply", "bucket"] = out["mlp_ppo_apply", "wide"] = apply_like(H.mlp_ppo_apply, False)
    out["mlp_ppo_apply_parts", "bucket"] = out["mlp_ppo_apply_parts", "wide"] = apply_like(H.mlp_ppo_apply_parts, True)
    out["head_ppo", "rec"] = out["head_ppo", "bucket"] = head
    out["mlp_layered_step", "rec"] = out["mlp_layered_step", "bucket"] = layered
    return out


BAD = _bad_cases()


@pytest.mark.parametrize("entry,what", sorted(BAD))
def test_a_mismatched_buffer_raises_before_the_library_is_reached(entry, what, monkeypatch):
    h = Harness()
    h.install(monkeypatch.setattr)
    with pytest.raises(ValueError):
        BAD[entry, what](h, what)
    assert h.calls == []


def _dump(transcripts):
    lines = []
    for name in sorted(transcripts):
        calls = ",\n".join("  " + json.dumps(c) for c in transcripts[name])
        lines.append(f"{json.dumps(name)}: [\n{calls}\n]")
    return "{\n" + ",\n".join(lines) + "\n}\n"


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

    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    result = {}
    for case_name in sorted(CASES):
        patch = _Patch()
        try:
            result[case_name] = run_case(case_name, patch.setattr)
        finally:
            patch.restore()
    os.makedirs(os.path.dirname(TRANSCRIPT), exist_ok=True)
    with open(TRANSCRIPT, "w") as f:
        f.write(_dump(result))
    print(f"{len(result)} cases, {sum(len(v) for v in result.values())} calls -> {TRANSCRIPT}")
