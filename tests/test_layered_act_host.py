"""CPU: the layered rollout step's cases (tests/layered_act_cases.py) and its host layer.  (1) For every case of the GPU test, ANOTHER
correct fp32 computation of the rollout step -- ``ref64.make_alternative_fp32_net``: exact six-product matrix products, the kernels'
tanh, a log-prob with 1 / (std * std) formed once -- meets the GPU test's bar against the CPU yardstick, and ``safe_uniform`` leaves no
draw within BRANCH_EPS of an edge: the bar can be met at these shapes without exclusions.  (2) What ``mlp_layered_prepare``,
``mlp_layered_act`` and ``head_act`` hand to the library equals tests/transcripts/layered_act_calls.json (the recorder of
tests/test_hip_ops_calls.py, imported), and mismatched buffers raise before the library is reached.

Re-record with ``python tests/test_layered_act_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import layered_act_cases as LA              # noqa: E402
from tests import ref64 as R                           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_act_calls.json")
N, A = 4, TC.A


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)       # fixed summation order in the CPU yardstick
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("c", LA.CASES, ids=LA.IDS)
def test_a_second_correct_fp32_formulation_meets_the_bar_at_the_layered_act_shapes(c, one_thread):
    data = LA.build(c)
    Y, y = LA.yardstick(c, data, "cpu")
    alt = R.make_alternative_fp32_net(data["sd"])
    m = LA.metrics(c, data["ref"], *LA.torch_fp32_step(c, data, "cpu", net=alt))
    print(f"\n[alternative fp32] {R.case_id(c)}: " + ", ".join(f"{n} {x:.3e} = {x / Y:.2f} x Y" for n, x in m.items()) + f" (Y {Y:.3e})")
    for n, x in m.items():
        assert x <= R.MARGIN * Y, (n, x, Y, x / Y)
    if not c.cont:
        # the second formulation samples the reference's index too: its CDF, as K14 forms it, against the safe draws
        with torch.no_grad():
            mu = alt.actor(data["obs"])
            lse = mu.max(1, keepdim=True).values + torch.log(torch.exp(mu - mu.max(1, keepdim=True).values).sum(1, keepdim=True))
            cdf = torch.exp(mu - lse).cumsum(1)
        pick = (data["noise"][:, None] >= cdf[:, :-1]).sum(1)
        assert torch.equal(pick, data["ref"]["action"])


@pytest.mark.parametrize("c", [c for c in LA.CASES if not c.cont], ids=[i for c, i in zip(LA.CASES, LA.IDS) if not c.cont])
def test_safe_uniform_leaves_no_draw_near_an_edge(c):
    data = LA.build(c)
    with torch.no_grad():
        cdf = torch.softmax(data["net64"].actor(data["obs"].double()), 1).cumsum(1)[:, :-1]
    near = ((data["noise"].double()[:, None] - cdf).abs() < R.BRANCH_EPS).any(1)
    assert int(near.sum()) == 0
    assert bool(((data["noise"] >= 0) & (data["noise"] < 1)).all())


@pytest.mark.parametrize("c", LA.CASES, ids=LA.IDS)
def test_every_case_is_a_layered_shape(c):
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    bucket = FlatBucket(pol.parameters())
    assert H.mlp_layout(pol, bucket) is None and H.mlp_layered_layout(pol, bucket) is not None


# ------------------------------------------------------------------ what the host layer hands to the library
CASES = {}


def _outs(h, cont):
    return (h.t("actions_out", N, A) if cont else h.t("actions_out", N)), h.t("logp", N), h.t("value", N)


def _act_case(kind, cont, mode):
    def run(h):
        lay, bucket, *_ = TC._mlp(h, kind, cont, False)
        obs = h.t("obs4", N, lay["D"])
        if mode == "value_only":
            a, lp, v = H.mlp_layered_act(obs, None, bucket.flat_param, lay)
            assert a is None and lp is None and v.shape == (N,)
            h.name("value_new", v)
            H.mlp_layered_act(obs, None, bucket.flat_param, lay, value=h.t("value", N))
        else:
            nz = h.t("noise", N, A) if cont else h.t("noise", N)
            if mode == "prepared":
                wop = H.mlp_layered_prepare(bucket.flat_param, lay)
                assert H.mlp_layered_prepare(bucket.flat_param, lay) is wop        # one buffer per (shape, device)
                assert wop.data_ptr() not in [w.data_ptr() for w in h.ws.values()]  # of its own: no shared workspace
                assert H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont), wop=wop)[0].shape == ((N, A) if cont else (N,))
            else:
                for n, o in zip(("actions_new", "logp_new", "value_new"), H.mlp_layered_act(obs, nz, bucket.flat_param, lay)):
                    assert o.shape == ((N, A) if cont and n == "actions_new" else (N,))
                    h.name(n, o)
                H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont))
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
    return run


def _head_case(cont, noise):
    def run(h):
        lay, bucket, *_ = TC._mlp(h, "layered3", cont, False)
        hA, hC = h.t("hA", N, 128), h.t("hC", N, 128)
        if not noise:
            a, lp, v = H.head_act(None, hC, None, bucket.flat_param, lay)
            assert a is None and lp is None
            h.name("value_new", v)
            H.head_act(hA, hC, None, bucket.flat_param, lay, value=h.t("value", N))
            return
        nz = h.t("noise", N, A) if cont else h.t("noise", N)
        for n, o in zip(("actions_new", "logp_new", "value_new"), H.head_act(hA, hC, nz, bucket.flat_param, lay)):
            h.name(n, o)
        H.head_act(hA, hC, nz, bucket.flat_param, lay, *_outs(h, cont))
    return run


for _kind, _cont in (("layered1", True), ("layered3", False)):
    for _mode in ("noise", "value_only", "prepared"):
        CASES[f"mlp_layered_act/{_kind}/{'continuous' if _cont else 'categorical'}/{_mode}"] = _act_case(_kind, _cont, _mode)
for _cont in (True, False):
    for _noise in (True, False):
        CASES[f"head_act/{'continuous' if _cont else 'categorical'}/{'noise' if _noise else 'value_only'}"] = _head_case(_cont, _noise)


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


def _bad(h, entry, what):
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
    if entry == "mlp_layered_act":
        H.mlp_layered_act(obs, nz, p, lay, a, lp, v)
    elif entry == "mlp_layered_prepare":
        H.mlp_layered_prepare(p, lay)
    else:
        hA, hC = h.t("hA", N, 128), h.t("hC", N, 128 if what != "obs" else 96)
        H.head_act(hA, hC, nz, p, lay, a, lp, v)


BAD = ([("mlp_layered_act", w) for w in ("obs", "noise", "actions", "logp", "value", "bucket", "layout")]
       + [("mlp_layered_prepare", w) for w in ("bucket", "layout")]
       + [("head_act", w) for w in ("obs", "noise", "actions", "logp", "value", "bucket")])


@pytest.mark.parametrize("entry,what", BAD)
def test_a_mismatched_buffer_raises_before_the_library_is_reached(entry, what, monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    H._layered_wop_cache.clear()
    with pytest.raises(ValueError):
        _bad(h, entry, what)
    assert h.calls == [] and not H._layered_wop_cache


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
