"""CPU: the host layer of the small-M products and the paired layered rollout step.  (1) What ``linear_small_bias_act``,
``linear_pair_bias_act`` and ``mlp_layered_act(paired=True)`` hand to the library equals
tests/transcripts/layered_act_paired_calls.json (the recorder of tests/test_hip_ops_calls.py, imported), and mismatched shapes raise
before the library is reached.  (2) The trainer's switch: unset, ``ppo`` passes no ``paired`` keyword at all; set without
``AURPPO_LAYERED_ACT`` it changes nothing; set with it, the rollout steps, the stand-alone step and the bootstrap all pass
``paired=True``.  (3) The new C entries refuse -- AURPPO_EINVAL / AURPPO_ESHAPE, nothing launched -- what their unpaired siblings refuse.

Re-record with ``python tests/test_layered_act_paired_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list
changes."""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import oracle_ops                           # noqa: E402
from tests import test_abi_signatures as SIG           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_act_paired_calls.json")
N, A, M = 4, TC.A, TC.M
EINVAL, ESHAPE = -1, -2
NEW = {"aurppo_linear_small_bias_act_f32": ("int", 10), "aurppo_linear_pair_wop_bytes": ("size_t", 2),
       "aurppo_linear_pair_bias_act_f32": ("int", 14), "aurppo_mlp_layered_act_paired_f32": ("int", 17)}


# ------------------------------------------------------------------ prototypes
@pytest.mark.parametrize("name", sorted(NEW))
def test_the_prototype_parses_and_the_binding_matches(name):
    import __graft_entry__ as g
    g.build()
    res, types_ = SIG.PROTOTYPES[name]
    assert (res, len(types_)) == NEW[name]
    fn = getattr(TC._lib.load(), name)
    assert len(fn.argtypes) == len(types_) and all(SIG._matches(t, d) for t, d in zip(fn.argtypes, types_))
    assert fn.restype is (C.c_size_t if res == "size_t" else C.c_int)


def test_the_new_entries_keep_their_siblings_argument_lists():
    P = SIG.PROTOTYPES
    assert P["aurppo_linear_small_bias_act_f32"][1] == P["aurppo_linear_bias_act_f32"][1]
    assert P["aurppo_mlp_layered_act_paired_f32"][1] == P["aurppo_mlp_layered_act_f32"][1]
    single = P["aurppo_linear_bias_act_f32"][1]                  # x, w, bias, y, then M ... stream
    assert P["aurppo_linear_pair_bias_act_f32"][1] == [t for t in single[:4] for _ in range(2)] + single[4:]


# ------------------------------------------------------------------ (1) what the host layer hands to the library
CASES = {}


def _small_case(h):
    h.name("y0", H.linear_small_bias_act(h.t("x", M, 16), h.t("w", 32, 16), h.t("bias", 32), act=1))
    h.name("y1", H.linear_small_bias_act(h.t("x2", M, 17), h.t("w2", 32, 17), None))


def _pair_case(shared):
    def run(h):
        xA = h.t("xA", M, 16)
        xC = xA if shared else h.t("xC", M, 16)
        yA, yC = H.linear_pair_bias_act(xA, xC, h.t("wA", 32, 16), h.t("wC", 32, 16), h.t("bA", 32), None if shared else h.t("bC", 32),
                                        act=0 if shared else 1)
        assert yA.shape == (M, 32) and yC.shape == (M, 32) and yA.data_ptr() != yC.data_ptr()
        h.name("yA", yA), h.name("yC", yC)
    return run


def _outs(h, cont):
    return (h.t("actions_out", N, A) if cont else h.t("actions_out", N)), h.t("logp", N), h.t("value", N)


def _act_case(kind, cont, mode):
    def run(h):
        lay, bucket, *_ = TC._mlp(h, kind, cont, False)
        obs = h.t("obs4", N, lay["D"])
        if mode == "value_only":
            a, lp, v = H.mlp_layered_act(obs, None, bucket.flat_param, lay, paired=True)
            assert a is None and lp is None and v.shape == (N,)
            h.name("value_new", v)
        else:
            nz = h.t("noise", N, A) if cont else h.t("noise", N)
            wop = H.mlp_layered_prepare(bucket.flat_param, lay) if mode == "prepared" else None
            got = H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont), wop=wop, paired=True)
            assert got[0].shape == ((N, A) if cont else (N,))
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
    return run


CASES["linear_small_bias_act"] = _small_case
CASES["linear_pair_bias_act/one_input"] = _pair_case(True)
CASES["linear_pair_bias_act/two_inputs"] = _pair_case(False)
for _kind, _cont in (("layered1", True), ("layered3", False)):
    for _mode in ("noise", "value_only", "prepared"):
        CASES[f"mlp_layered_act_paired/{_kind}/{'continuous' if _cont else 'categorical'}/{_mode}"] = _act_case(_kind, _cont, _mode)


def run_case(name, setattr_, bound=None):
    h = TC.Harness(bound)
    h.install(setattr_)
    setattr_(torch.cuda, "current_device", lambda: 0)
    H._layered_wop_cache.clear()
    try:
        CASES[name](h)
        return json.loads(json.dumps(h.transcript()))
    finally:
        H._layered_wop_cache.clear()


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
    """The same cases against the real binding's ``argtypes`` (count and ctypes conversion; nothing is launched)."""
    import __graft_entry__ as g
    g.build()
    bound = TC._lib.load()
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


def test_the_paired_call_differs_from_the_unpaired_one_in_the_entry_alone(monkeypatch):
    """Same size queries, same workspace, same seventeen arguments: only the function's name changes; the default is the old call."""
    def calls(**kw):
        h = TC.Harness()
        h.install(monkeypatch.setattr)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        H._layered_wop_cache.clear()
        lay, bucket, *_ = TC._mlp(h, "layered3", True, False)
        H.mlp_layered_act(h.t("obs4", N, lay["D"]), h.t("noise", N, A), bucket.flat_param, lay, *_outs(h, True), **kw)
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
        H._layered_wop_cache.clear()
        return json.loads(json.dumps(h.transcript()))
    plain, off, on = calls(), calls(paired=False), calls(paired=True)
    assert plain == off and plain[-1][0] == "aurppo_mlp_layered_act_f32" and on[-1][0] == "aurppo_mlp_layered_act_paired_f32"
    assert on[:-1] == plain[:-1] and on[-1][1] == plain[-1][1] and len(on[-1][1]) == 17


def _bad(h, entry, what):
    if entry == "linear_small_bias_act":
        x, w, b = h.t("x", M, 16), h.t("w", 32, 16), h.t("bias", 32)
        if what == "x":
            x = h.t("x_wide", M, 32)
        elif what == "bias":
            b = h.t("bias_short", 31)
        H.linear_small_bias_act(x, w, b)
    else:
        xA, xC, wA, wC, bA, bC = h.t("xA", M, 16), h.t("xC", M, 16), h.t("wA", 32, 16), h.t("wC", 32, 16), h.t("bA", 32), h.t("bC", 32)
        if what == "rows":
            xC = h.t("xC_short", M - 1, 16)
        elif what == "x":
            xA = xC = h.t("x_wide", M, 32)
        elif what == "w":
            wC = h.t("wC_tall", 64, 16)
        elif what == "bias":
            bC = h.t("bC_long", 33)
        H.linear_pair_bias_act(xA, xC, wA, wC, bA, bC)


BAD = [("linear_small_bias_act", w) for w in ("x", "bias")] + [("linear_pair_bias_act", w) for w in ("rows", "x", "w", "bias")]


@pytest.mark.parametrize("entry,what", BAD)
def test_a_mismatched_shape_raises_before_the_library_is_reached(entry, what, monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    with pytest.raises(ValueError):
        _bad(h, entry, what)
    assert h.calls == []


@pytest.mark.parametrize("what", ["obs", "noise", "actions", "logp", "value", "bucket", "layout"])
def test_a_mismatched_buffer_of_the_paired_act_raises_before_the_library_is_reached(what, monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    H._layered_wop_cache.clear()
    lay, bucket, *_ = TC._mlp(h, "layered3", True, False)
    obs, nz = h.t("obs4", N, lay["D"]), h.t("noise", N, A)
    a, lp, v = _outs(h, True)
    p = bucket.flat_param
    if what == "obs":
        obs = h.t("obs_wide", N, lay["D"] + 16)
    elif what == "noise":
        nz = h.t("noise_short", N, A - 1)
    elif what == "actions":
        a = h.t("actions_short", N - 1, A)
    elif what == "logp":
        lp = h.t("logp_long", N + 1)
    elif what == "value":
        v = h.t("value_long", N + 1)
    elif what == "bucket":
        p = h.t("short", lay["n_params"] - 1)
    elif what == "layout":
        lay = dict(lay, layered=False)
    with pytest.raises(ValueError):
        H.mlp_layered_act(obs, nz, p, lay, a, lp, v, paired=True)
    assert h.calls == [] and not H._layered_wop_cache


# ------------------------------------------------------------------ (2) the trainer's switch
def _params(**over):
    p = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=3, gae=True, total_timesteps=48, anneal_lr=True, gae_lambda=0.95,
             num_update_epochs=1, num_envs=8, num_minibatches=2, entropy_coeff=0.0, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True,
             max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=256, continuous=True,
             learning_rate=3e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False, save=False,
             obs_dim=16, act_dim=3, device="cpu")
    p.update(over)
    return p


def _recording_ops(log):
    """The oracle's ops with a layered rollout step that records its keywords and writes zeros."""
    ops = types.SimpleNamespace(**{k: getattr(oracle_ops, k) for k in dir(oracle_ops) if not k.startswith("__")})

    def mlp_layered_act(obs, noise, flat_param, layout, actions=None, logp=None, value=None, **kw):
        log.append(("act", noise is not None, dict(kw)))
        n = obs.shape[0]
        value = torch.zeros(n) if value is None else value.zero_()
        if noise is None:
            return None, None, value
        return actions.zero_(), logp.zero_(), value

    def mlp_layered_prepare(flat_param, layout):
        log.append(("prepare",))
        return torch.zeros(1)
    ops.mlp_layered_act, ops.mlp_layered_prepare = mlp_layered_act, mlp_layered_prepare
    ops.mlp_layered_layout = H.mlp_layered_layout
    return ops


def _cpu_agent(log):
    """A CPU agent (the layered switches are read on a GPU only) given the layered act layout by hand, the paired flag by the
    trainer's own rule."""
    from aur_ppo_amd import ppo as P
    a = P.ppo(_params(), ops=_recording_ops(log))
    assert a._mlp is None and a._mlp_layered_act is None and a._act_paired is False        # no GPU: no switch is on
    a._mlp_layered_act = H.mlp_layered_layout(a.policy, a.bucket, any_state=True)
    assert a._mlp_layered_act is not None
    a._act_paired = P._layered_act_paired(a._mlp_layered_act)
    return a


def _one_rollout(a):
    obs = torch.as_tensor(a.envs.reset(seed=list(range(a.num_envs)))[0], dtype=torch.float32)
    done = torch.zeros(a.num_envs)
    obs, done, _ = a._rollout_steps(obs, done, 0, None)
    a.rewards_to_go(0, obs, 0, None)              # a stand-alone step
    a.advantages(obs, done)                       # the bootstrap


def test_the_switch_is_off_by_default_and_read_only_beside_the_layered_act(monkeypatch):
    from aur_ppo_amd import ppo as P
    assert P.LAYERED_ACT_PAIRED_DEFAULT == "0"
    lay = {"layered": True}
    monkeypatch.delenv("AURPPO_LAYERED_ACT_PAIRED", raising=False)
    assert P._layered_act_paired(lay) is False and P._layered_act_paired(None) is False
    monkeypatch.setenv("AURPPO_LAYERED_ACT_PAIRED", "0")
    assert P._layered_act_paired(lay) is False
    monkeypatch.setenv("AURPPO_LAYERED_ACT_PAIRED", "1")
    assert P._layered_act_paired(lay) is True and P._layered_act_paired(None) is False     # alone it changes nothing


def test_unset_the_trainer_passes_no_paired_keyword(monkeypatch):
    monkeypatch.delenv("AURPPO_LAYERED_ACT_PAIRED", raising=False)
    log = []
    a = _cpu_agent(log)
    assert a._act_paired is False
    _one_rollout(a)
    acts = [e for e in log if e[0] == "act"]
    assert len(acts) == a.num_steps + 2 and [e[1] for e in acts] == [True] * (a.num_steps + 1) + [False]
    assert all(sorted(e[2]) == ["wop"] for e in acts)           # the call is what it was, keyword for keyword


def test_set_the_trainer_passes_paired_in_the_rollout_the_step_and_the_bootstrap(monkeypatch):
    monkeypatch.setenv("AURPPO_LAYERED_ACT_PAIRED", "1")
    log = []
    a = _cpu_agent(log)
    assert a._act_paired is True
    _one_rollout(a)
    acts = [e for e in log if e[0] == "act"]
    assert len(acts) == a.num_steps + 2 and [e[1] for e in acts] == [True] * (a.num_steps + 1) + [False]
    assert all(sorted(e[2]) == ["paired", "wop"] and e[2]["paired"] is True for e in acts)
    assert [e[2]["wop"] is not None for e in acts] == [True] * a.num_steps + [False, False]     # prepared once per rollout


def test_the_switch_alone_leaves_the_torch_route(monkeypatch):
    """``AURPPO_LAYERED_ACT_PAIRED=1`` without ``AURPPO_LAYERED_ACT``: no act layout, ``policy.evaluate`` runs, nothing is recorded."""
    from aur_ppo_amd import ppo as P
    monkeypatch.setenv("AURPPO_LAYERED_ACT_PAIRED", "1")
    monkeypatch.delenv("AURPPO_LAYERED_ACT", raising=False)
    log = []
    a = P.ppo(_params(), ops=_recording_ops(log))
    assert a._mlp_layered_act is None and a._act_paired is False and a._act_layout() is None
    calls = []
    evaluate = a.policy.evaluate
    monkeypatch.setattr(a.policy, "evaluate", lambda *args, **kw: calls.append(1) or evaluate(*args, **kw))
    obs = torch.as_tensor(a.envs.reset(seed=list(range(a.num_envs)))[0], dtype=torch.float32)
    a.rewards_to_go(0, obs, 0, None)
    assert calls == [1] and log == []


# ------------------------------------------------------------------ (3) the C entries refuse before any launch
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return TC._lib.load()


def _fake(offset=0):
    """A host buffer's address (+ offset): the entries under test refuse before anything dereferences or launches."""
    buf = (C.c_float * 4096)()
    _fake.keep.append(buf)
    base = C.addressof(buf)
    return C.c_void_p(base + (-base % 64) + offset)


_fake.keep = []


def test_the_small_product_refuses_without_a_launch(lib):
    p = _fake()
    ok = dict(x=p, w=p, bias=p, y=p, M=4, K=16, N=32, act=1, ws=p)

    def call(**over):
        a = dict(ok, **over)
        return lib.aurppo_linear_small_bias_act_f32(a["x"], a["w"], a["bias"], a["y"], a["M"], a["K"], a["N"], a["act"], a["ws"], None)
    assert call(M=0) == ESHAPE and b"M=0" in lib.aurppo_last_error()
    assert call(K=0) == ESHAPE and call(N=0) == ESHAPE
    assert call(act=2) == EINVAL and b"act 2" in lib.aurppo_last_error()
    for name in ("x", "w", "y", "ws"):
        assert call(**{name: None}) == EINVAL and b"null pointer" in lib.aurppo_last_error(), name
    assert call(x=_fake(4)) == EINVAL and b"aligned" in lib.aurppo_last_error()
    assert call(ws=_fake(8)) == EINVAL


def test_the_paired_product_refuses_without_a_launch(lib):
    p = _fake()
    names = ("xA", "xC", "wA", "wC", "biasA", "biasC", "yA", "yC")
    ok = dict({n: p for n in names}, M=4, K=16, N=32, act=1, ws=p)

    def call(**over):
        a = dict(ok, **over)
        return lib.aurppo_linear_pair_bias_act_f32(*[a[n] for n in names], a["M"], a["K"], a["N"], a["act"], a["ws"], None)
    assert call(M=0) == ESHAPE and call(K=0) == ESHAPE and call(N=0) == ESHAPE
    assert call(act=2) == EINVAL and b"act 2" in lib.aurppo_last_error()
    for name in ("xA", "xC", "wA", "wC", "yA", "yC", "ws"):
        assert call(**{name: None}) == EINVAL and b"null pointer" in lib.aurppo_last_error(), name
    assert call(xA=_fake(4)) == EINVAL and call(xC=_fake(4)) == EINVAL and b"aligned" in lib.aurppo_last_error()
    assert lib.aurppo_linear_pair_wop_bytes(0, 32) == 0 and lib.aurppo_linear_pair_wop_bytes(16, 0) == 0
    for K, Nw in [(16, 32), (17, 256), (376, 64), (256, 1024)]:
        one = (-(-Nw // 32) + 4) * -(-K // 16) * 3 * 1024          # the blocks of one operand copy and a group of slack
        assert lib.aurppo_linear_pair_wop_bytes(K, Nw) == 2 * one


def test_the_paired_act_refuses_what_the_unpaired_act_refuses(lib):
    p = _fake()
    L, D, Hd, A_ = 2, 64, 256, 6
    n_params = 2 * (D * Hd + Hd + Hd * Hd + Hd) + (A_ * Hd + A_) + (Hd + 1) + A_
    offsets = []
    at = 0
    for out in (A_, 1):
        for l in range(L + 1):
            o, k = (Hd if l < L else out), (D if l == 0 else Hd)
            offsets += [at, at + o * k]
            at += o * k + o
    offsets.append(at)
    assert at + A_ == n_params and len(offsets) == 4 * (L + 1) + 1
    ok = dict(obs=p, noise=p, N=4, D=D, A=A_, cont=1, hidden=Hd, L=L, params=p, offsets=offsets, n_params=n_params, actions=p, logp=p,
              value=p, wop=p, ws=p)

    def call(entry, **over):
        a = dict(ok, **over)
        off = (C.c_int * len(a["offsets"]))(*a["offsets"]) if a["offsets"] is not None else None
        return getattr(lib, entry)(a["obs"], a["noise"], a["N"], a["D"], a["A"], a["cont"], a["hidden"], a["L"], a["params"], off,
                                   a["n_params"], a["actions"], a["logp"], a["value"], a["wop"], a["ws"], None)
    outside = list(offsets)
    outside[3] = n_params - 8                      # the actor's second bias: 256 floats from 8 short of the end
    for over, rc, word in [(dict(N=0), ESHAPE, b"N=0"), (dict(D=0), ESHAPE, b"D=0"), (dict(hidden=48), ESHAPE, b"hidden=48"),
                           (dict(L=0), ESHAPE, b"layers"), (dict(L=17), ESHAPE, b"layers"), (dict(A=17), ESHAPE, b"A=17"),
                           (dict(obs=None), EINVAL, b"null pointer"), (dict(value=None), EINVAL, b"null pointer"),
                           (dict(wop=None), EINVAL, b"null pointer"), (dict(ws=None), EINVAL, b"null pointer"),
                           (dict(offsets=None), EINVAL, b"null pointer"), (dict(actions=None), EINVAL, b"null pointer"),
                           (dict(obs=_fake(4)), EINVAL, b"aligned"), (dict(ws=_fake(16)), EINVAL, b"aligned"),
                           (dict(offsets=outside), EINVAL, b"outside the bucket")]:
        got = call("aurppo_mlp_layered_act_paired_f32", **over)
        msg = lib.aurppo_last_error()
        assert got == rc and word in msg and b"aurppo_mlp_layered_act_paired_f32" in msg, (over.keys(), got, msg)
        assert call("aurppo_mlp_layered_act_f32", **over) == rc                      # its sibling: the same refusal


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
