"""CPU: the layered routes at hidden widths that are no multiple of 32 (tests/layered_hidden_cases.py).  (1) For every case of the GPU
test, ANOTHER correct fp32 computation -- ``ref64.make_alternative_fp32_net`` -- meets the same bars against the CPU yardstick, for the
step and for the rollout step (the bodies of tests/test_layered_ragged_host.py part (1)): the bars the GPU test holds the kernels to can
be met at these shapes without exclusions.  (2) Which policies ``hip_ops.mlp_layered_layout`` takes with ``any_hidden=True`` and which it
still refuses (it needs no device).  (3) What ``mlp_layered_step_native``, ``mlp_layered_minibatch``, ``mlp_layered_prepare`` and
``mlp_layered_act`` (unpaired, paired, value-only) hand to the library at 2 x 200 over D = 17 equals
tests/transcripts/layered_hidden_calls.json (the recorder of tests/test_hip_ops_calls.py, imported): the ``anyh`` entries, with the
siblings' arguments and ``hidden`` as it is.  (4) The size functions round the width up to 32.  (5) Every ``anyh`` entry refuses what its
sibling refuses, with nothing launched.  (6) The per-product Python route refuses a ragged-hidden layout.  (7) The trainer's switch and
its route choice.

Re-record with ``python tests/test_layered_hidden_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
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

from tests import layered_act_cases as LA              # noqa: E402
from tests import layered_hidden_cases as LH           # noqa: E402
from tests import oracle_ops                           # noqa: E402
from tests import ref64 as R                           # noqa: E402
from tests import test_abi_signatures as SIG           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_hidden_calls.json")
N, A, D, HIDDEN, LAYERS = 4, TC.A, 17, 200, 2
M, B = TC.M, TC.B
EINVAL, ESHAPE = -1, -2
SIBLINGS = {"aurppo_mlp_layered_anyh_" + n: "aurppo_mlp_layered_" + n
            for n in ("step_workspace_bytes", "step_f32", "minibatch_f32", "wop_bytes", "prep_f32", "act_workspace_bytes", "act_f32",
                      "act_paired_f32")}


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)       # fixed summation order in the CPU yardstick
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return TC._lib.load()


# ------------------------------------------------------------------ (1) the bars can be met at these shapes
@pytest.mark.parametrize("c", LH.STEP_CASES, ids=LH.STEP_IDS)
def test_a_second_correct_fp32_formulation_meets_the_bars_at_the_ragged_hidden_step_shapes(c, one_thread):
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cpu")
    li = data["idx"].long()
    got = R.run_step(R.make_alternative_fp32_net(data["sd"]), data["obs"][li], data["act"][li] if c.cont else data["act"][li].long(),
                     data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    R.check_step(c, got["scalars"], got["flat"], data["ref"], Y, Ys, "alternative fp32")


@pytest.mark.parametrize("c", LH.ACT_CASES, ids=LH.ACT_IDS)
def test_a_second_correct_fp32_formulation_meets_the_bar_at_the_ragged_hidden_act_shapes(c, one_thread):
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


# ------------------------------------------------------------------ (2) the layout rule
def _layouts(hidden, layers, D_, A_, cont=True, **kw):
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(D_, (A_,) if cont else A_, hidden, layers, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    return H.mlp_layout(pol, bucket), H.mlp_layered_layout(pol, bucket, **kw)


@pytest.mark.parametrize("hidden,layers,D_,A_", [(200, 2, 17, 6), (100, 1, 376, 16), (5, 3, 129, 6)])
def test_any_hidden_gives_a_ragged_width_a_layered_layout_of_the_unpadded_policy(hidden, layers, D_, A_):
    fused, lay = _layouts(hidden, layers, D_, A_, any_state=True, any_hidden=True)
    assert fused is None and isinstance(lay, dict) and lay["layered"] is True and lay["ragged_hidden"] is True
    assert (lay["hidden"], lay["num_layers"], lay["D"], lay["A"], lay["continuous"]) == (hidden, layers, D_, A_, True)
    assert len(lay["offsets"]) == 4 * (layers + 1) + 1 and len(H.head_layout(lay)) == 7
    n_w = sum((D_ * hidden + hidden) + (layers - 1) * (hidden * hidden + hidden) + (out * hidden + out) for out in (A_, 1))
    assert lay["n_params"] == n_w + A_                  # nothing of the padded width is in the bucket
    # without the keyword, and with any_state alone, these stay refused
    assert _layouts(hidden, layers, D_, A_)[1] is None and _layouts(hidden, layers, D_, A_, any_state=True)[1] is None
    assert _layouts(hidden, layers, D_, A_, any_state=True, any_hidden=False)[1] is None


def test_an_aligned_width_keeps_its_layout_under_any_hidden():
    _fused, lay = _layouts(256, 2, 17, 6, any_state=True, any_hidden=True)
    assert lay is not None and "ragged_hidden" not in lay
    assert lay == _layouts(256, 2, 17, 6, any_state=True)[1]
    assert _layouts(256, 2, 17, 6)[1] is None           # (the ragged state still needs its own keyword)


@pytest.mark.parametrize("hidden,layers,D_,A_", [(1025, 2, 17, 6), (200, 2, 17, 17), (1056, 2, 17, 6)])
def test_any_hidden_drops_the_multiple_of_32_condition_only(hidden, layers, D_, A_):
    """A hidden width past 1024, 17 actions: no layered layout with the keyword or without it."""
    assert _layouts(hidden, layers, D_, A_, any_state=True, any_hidden=True)[1] is None
    assert _layouts(hidden, layers, D_, A_)[1] is None


def test_any_hidden_alone_still_needs_a_state_of_whole_k_steps():
    assert _layouts(200, 2, 17, 6, any_hidden=True)[1] is None
    assert _layouts(200, 2, 16, 6, any_hidden=True)[1]["ragged_hidden"] is True


@pytest.mark.parametrize("hidden,layers,D_,A_", [(64, 2, 17, 6), (100, 2, 17, 6), (128, 3, 128, 6), (33, 3, 128, 6)])
def test_the_fused_kernels_shapes_stay_with_them_under_any_hidden(hidden, layers, D_, A_):
    fused, layered = _layouts(hidden, layers, D_, A_, any_state=True, any_hidden=True)
    assert fused is not None and layered is None


@pytest.mark.parametrize("c", LH.STEP_CASES + LH.ACT_CASES, ids=["step-" + i for i in LH.STEP_IDS] + ["act-" + i for i in LH.ACT_IDS])
def test_every_case_is_a_ragged_hidden_layered_shape(c):
    fused, lay = _layouts(c.hidden, c.layers, c.D, c.A, c.cont, any_state=True, any_hidden=True)
    assert fused is None and lay is not None and lay["ragged_hidden"] is True and c.hidden % 32 != 0
    assert _layouts(c.hidden, c.layers, c.D, c.A, c.cont, any_state=True)[1] is None


# ------------------------------------------------------------------ (3) what the host layer hands to the library at 2 x 200 over D = 17
CASES = {}


def _ragged(h, cont, packed):
    """(layout, bucket, obs, actions, rec, idx) of a 2 x 200 policy over a state of 17 floats, its layout through ``any_hidden``."""
    pol, bucket = TC._policy(h, D, HIDDEN, LAYERS, cont)
    assert H.mlp_layered_layout(pol, bucket, any_state=True) is None
    lay = H.mlp_layered_layout(pol, bucket, any_state=True, any_hidden=True)
    assert lay["D"] == D and lay["hidden"] == HIDDEN and lay["ragged_hidden"] and lay["offsets"][2] != 0 and lay["continuous"] == cont
    obs = h.t("obs", B, D)
    if packed:
        actions, rec = None, h.t("rec64", B, 16)
    else:
        actions, rec = (h.t("actions", B, A) if cont else h.t("actions", B)), h.t("rec", B, 4)
    return lay, bucket, obs, actions, rec, h.idx("idx")


def _step_case(cont, packed, minibatch):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _ragged(h, cont, packed)
        sc = h.t("scalars", 9)
        if minibatch:
            m, v, lr, step, norms = TC._adam(h, bucket)
            assert H.mlp_layered_minibatch(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True,
                                           H.VLOSS_CLIPPED, sc, m, v, lr, step, TC.MAX_NORM, TC.BETAS, TC.EPS, norms[1:2]) is sc
        else:
            assert H.mlp_layered_step_native(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True,
                                             H.VLOSS_OLDVALUES, sc) is sc
    return run


def _outs(h, cont):
    return (h.t("actions_out", N, A) if cont else h.t("actions_out", N)), h.t("logp", N), h.t("value", N)


def _act_case(cont, mode, paired):
    def run(h):
        lay, bucket, *_ = _ragged(h, cont, False)
        obs = h.t("obs4", N, D)
        kw = dict(paired=True) if paired else {}
        if mode == "value_only":
            a, lp, v = H.mlp_layered_act(obs, None, bucket.flat_param, lay, **kw)
            assert a is None and lp is None and v.shape == (N,)
            h.name("value_new", v)
        else:
            nz = h.t("noise", N, A) if cont else h.t("noise", N)
            wop = H.mlp_layered_prepare(bucket.flat_param, lay)
            assert H.mlp_layered_prepare(bucket.flat_param, lay) is wop
            assert H.mlp_layered_act(obs, nz, bucket.flat_param, lay, *_outs(h, cont), wop=wop, **kw)[0].shape == ((N, A) if cont else (N,))
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
    return run


CASES["mlp_layered_step_native/2x200/continuous/packed"] = _step_case(True, True, False)
CASES["mlp_layered_step_native/2x200/categorical"] = _step_case(False, False, False)
CASES["mlp_layered_minibatch/2x200/continuous/packed"] = _step_case(True, True, True)
CASES["mlp_layered_act/2x200/continuous/prepared"] = _act_case(True, "prepared", False)
CASES["mlp_layered_act/2x200/categorical/prepared/paired"] = _act_case(False, "prepared", True)
CASES["mlp_layered_act/2x200/continuous/value_only"] = _act_case(True, "value_only", False)
CASES["mlp_layered_act/2x200/continuous/value_only/paired"] = _act_case(True, "value_only", True)


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


def test_the_entries_are_the_anyh_ones_and_the_width_reaches_them_as_it_is():
    """Every library call of every case is an ``anyh`` entry, ``hidden`` arrives as 200 (not 224), and the workspaces are the width's own."""
    where = {"step_workspace_bytes": 3, "step_f32": 8, "minibatch_f32": 8, "wop_bytes": 1, "prep_f32": 4, "act_workspace_bytes": 1,
             "act_f32": 6, "act_paired_f32": 6}
    seen = set()
    for name, calls in _recorded().items():
        for fn, args in calls:
            if fn == "_workspace":
                assert args[0] in ("layered_step_h200", "layered_act_h200"), (name, args)
                continue
            assert fn in SIBLINGS, (name, fn)
            short = fn[len("aurppo_mlp_layered_anyh_"):]
            assert args[where[short]] == HIDDEN, (name, fn, args)
            seen.add(short)
    assert seen == set(where)


def test_an_anyh_call_differs_from_its_sibling_in_the_entry_and_the_workspace_key_alone(monkeypatch):
    """The same policy's layout with and without ``ragged_hidden``: same arguments in the same order, call for call."""
    def calls(ragged):
        h = TC.Harness()
        h.install(monkeypatch.setattr)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        H._layered_wop_cache.clear()
        lay, bucket, obs, actions, rec, idx = _ragged(h, True, True)
        if not ragged:
            del lay["ragged_hidden"]
        H.mlp_layered_step_native(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True,
                                  H.VLOSS_CLIPPED, h.t("scalars", 9))
        H.mlp_layered_act(h.t("obs4", N, D), h.t("noise", N, A), bucket.flat_param, lay, *_outs(h, True), paired=True)
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
        H._layered_wop_cache.clear()
        return json.loads(json.dumps(h.transcript()))
    on, off = calls(True), calls(False)
    assert len(on) == len(off) > 0
    for (fa, aa), (fb, ab) in zip(on, off):
        if fa == "_workspace":
            assert fb == "_workspace" and aa[0] == ab[0] + "_h200" and aa[1] == ab[1]
        else:
            assert SIBLINGS[fa] == fb and [str(x).replace("_h200", "") for x in aa] == [str(x) for x in ab]


def test_every_call_fits_the_bound_argtypes(monkeypatch, lib):
    """The same cases against the real binding's ``argtypes`` (count and ctypes conversion; nothing is launched)."""
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, lib)


@pytest.mark.parametrize("name", sorted(SIBLINGS))
def test_the_prototype_parses_and_is_its_siblings(name, lib):
    res, types_ = SIG.PROTOTYPES[name]
    assert (res, types_) == SIG.PROTOTYPES[SIBLINGS[name]]
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(types_) and all(SIG._matches(t, d) for t, d in zip(fn.argtypes, types_))
    assert fn.restype is (C.c_size_t if res == "size_t" else C.c_int)


# ------------------------------------------------------------------ (4) the size functions
def test_the_size_functions_round_the_hidden_width_up_to_32(lib):
    for D_, L in ((17, 2), (376, 1), (16, 3)):
        at_224 = lib.aurppo_mlp_layered_anyh_wop_bytes(D_, 224, L)
        assert at_224 == lib.aurppo_mlp_layered_wop_bytes(D_, 224, L) > 0
        for h in range(193, 225):
            assert lib.aurppo_mlp_layered_anyh_wop_bytes(D_, h, L) == at_224, h
            assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(257, D_, 6, h, L) == lib.aurppo_mlp_layered_step_workspace_bytes(257, D_, 6, 224, L) > 0
            assert lib.aurppo_mlp_layered_anyh_act_workspace_bytes(65, h) == lib.aurppo_mlp_layered_act_workspace_bytes(65, 224) > 0
    for h in (32, 64, 256, 1024):
        assert lib.aurppo_mlp_layered_anyh_wop_bytes(17, h, 2) == lib.aurppo_mlp_layered_wop_bytes(17, h, 2) > 0
        assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(1000, 17, 6, h, 2) == lib.aurppo_mlp_layered_step_workspace_bytes(1000, 17, 6, h, 2) > 0
        assert lib.aurppo_mlp_layered_anyh_act_workspace_bytes(1000, h) == lib.aurppo_mlp_layered_act_workspace_bytes(1000, h) > 0
    for h in (1, 5, 31, 48, 1000):
        assert lib.aurppo_mlp_layered_anyh_wop_bytes(17, h, 2) > 0 and lib.aurppo_mlp_layered_anyh_step_workspace_bytes(65, 17, 6, h, 2) > 0
        assert lib.aurppo_mlp_layered_anyh_act_workspace_bytes(65, h) > 0
    for h in (0, 1025, -32):
        assert lib.aurppo_mlp_layered_anyh_wop_bytes(17, h, 2) == 0
        assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(65, 17, 6, h, 2) == 0
        assert lib.aurppo_mlp_layered_anyh_act_workspace_bytes(65, h) == 0
    # the siblings refuse what they refused
    assert lib.aurppo_mlp_layered_wop_bytes(17, 100, 2) == 0 and lib.aurppo_mlp_layered_step_workspace_bytes(65, 17, 6, 200, 2) == 0
    # what else the siblings' size functions refuse
    assert lib.aurppo_mlp_layered_anyh_wop_bytes(0, 200, 2) == 0 and lib.aurppo_mlp_layered_anyh_wop_bytes(17, 200, 0) == 0
    assert lib.aurppo_mlp_layered_anyh_wop_bytes(17, 200, 17) == 0 and lib.aurppo_mlp_layered_anyh_act_workspace_bytes(0, 200) == 0
    assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(0, 17, 6, 200, 2) == 0 and lib.aurppo_mlp_layered_anyh_step_workspace_bytes(65, 17, 17, 200, 2) == 0
    assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(65, 0, 6, 200, 2) == 0 and lib.aurppo_mlp_layered_anyh_step_workspace_bytes(65, 17, 6, 200, 17) == 0


# ------------------------------------------------------------------ (5) the C entries refuse before any launch
def _fake(offset=0):
    """A host buffer's address (+ offset): the entries under test refuse before anything dereferences or launches."""
    buf = (C.c_float * 4096)()
    _fake.keep.append(buf)
    base = C.addressof(buf)
    return C.c_void_p(base + (-base % 64) + offset)


_fake.keep = []


def _offsets(D_, Hd, L, A_):
    offsets, at = [], 0
    for out in (A_, 1):
        for l in range(L + 1):
            o, k = (Hd if l < L else out), (D_ if l == 0 else Hd)
            offsets += [at, at + o * k]
            at += o * k + o
    offsets.append(at)
    return offsets, at + A_


@pytest.mark.parametrize("entry", ["act_f32", "act_paired_f32"])
def test_the_anyh_act_refuses_what_its_sibling_refuses(entry, lib):
    p = _fake()
    L, D_, Hd, A_ = 2, 64, 200, 6
    offsets, n_params = _offsets(D_, Hd, L, A_)
    ok = dict(obs=p, noise=p, N=4, D=D_, A=A_, cont=1, hidden=Hd, L=L, params=p, offsets=offsets, n_params=n_params, actions=p, logp=p,
              value=p, wop=p, ws=p)

    def call(name, **over):
        a = dict(ok, **over)
        off = (C.c_int * len(a["offsets"]))(*a["offsets"]) if a["offsets"] is not None else None
        return getattr(lib, name)(a["obs"], a["noise"], a["N"], a["D"], a["A"], a["cont"], a["hidden"], a["L"], a["params"], off,
                                  a["n_params"], a["actions"], a["logp"], a["value"], a["wop"], a["ws"], None)
    outside = list(offsets)
    outside[3] = n_params - 8                      # the actor's second bias: 200 floats from 8 short of the end
    name = "aurppo_mlp_layered_anyh_" + entry
    for over, rc, word in [(dict(N=0), ESHAPE, b"N=0"), (dict(D=0), ESHAPE, b"D=0"), (dict(hidden=0), ESHAPE, b"hidden=0"),
                           (dict(hidden=1025), ESHAPE, b"hidden=1025"), (dict(hidden=-32), ESHAPE, b"hidden=-32"),
                           (dict(L=0), ESHAPE, b"layers"), (dict(L=17), ESHAPE, b"layers"), (dict(A=17), ESHAPE, b"A=17"),
                           (dict(A=1, cont=0), ESHAPE, b"A=1"),
                           (dict(obs=None), EINVAL, b"null pointer"), (dict(value=None), EINVAL, b"null pointer"),
                           (dict(wop=None), EINVAL, b"null pointer"), (dict(ws=None), EINVAL, b"null pointer"),
                           (dict(offsets=None), EINVAL, b"null pointer"), (dict(actions=None), EINVAL, b"null pointer"),
                           (dict(params=None), EINVAL, b"null pointer"),
                           (dict(obs=_fake(4)), EINVAL, b"aligned"), (dict(ws=_fake(16)), EINVAL, b"aligned"), (dict(wop=_fake(8)), EINVAL, b"aligned"),
                           (dict(value=_fake(2)), EINVAL, b"aligned"),
                           (dict(offsets=outside), EINVAL, b"outside the bucket"), (dict(n_params=n_params - 1), EINVAL, b"outside the bucket")]:
        got = call(name, **over)
        msg = lib.aurppo_last_error()
        assert got == rc and word in msg and name.encode() in msg, (list(over), got, msg)
        if "hidden" not in over:                   # its sibling at the aligned width next door: the same refusal
            offs_224, n_224 = _offsets(D_, 224, L, A_)
            sib = dict(hidden=224, offsets=offs_224, n_params=n_224)
            if "offsets" in over and over["offsets"] is not None:
                sib["offsets"] = offs_224[:3] + [n_224 - 8] + offs_224[4:]
            if "n_params" in over:
                sib["n_params"] = n_224 - 1
            sib.update({k: v for k, v in over.items() if k not in ("offsets", "n_params") or v is None})
            assert call(SIBLINGS[name], **sib) == rc, list(over)
    assert call(SIBLINGS[name], hidden=48) == ESHAPE and b"hidden=48" in lib.aurppo_last_error()     # what the old entries still refuse


@pytest.mark.parametrize("entry", ["step_f32", "minibatch_f32"])
def test_the_anyh_step_refuses_what_its_sibling_refuses(entry, lib):
    p = _fake()
    L, D_, Hd, A_ = 2, 17, 200, 6
    offsets, n_params = _offsets(D_, Hd, L, A_)
    ok = dict(obs=p, actions=p, rec=p, idx=p, M=4, D=D_, A=A_, cont=1, hidden=Hd, L=L, params=p, offsets=offsets, n_params=n_params,
              grads=p, vmode=1, sc=p, m=p, v=p, lr=p, t=p, norm=p, ws=p)

    def call(name, **over):
        a = dict(ok, **over)
        off = (C.c_int * len(a["offsets"]))(*a["offsets"]) if a["offsets"] is not None else None
        args = [a["obs"], a["actions"], a["rec"], a["idx"], a["M"], a["D"], a["A"], a["cont"], a["hidden"], a["L"], a["params"], off,
                a["n_params"], a["grads"], 0.2, 0.01, 0.5, 1, a["vmode"], a["sc"]]
        if name.endswith("minibatch_f32"):
            args += [a["m"], a["v"], 0.5, a["lr"], a["t"], 0.9, 0.999, 1e-5, a["norm"]]
        return getattr(lib, name)(*args, a["ws"], None)
    outside = list(offsets)
    outside[1] = n_params - 8                      # the actor's first bias: 200 floats from 8 short of the end
    name = "aurppo_mlp_layered_anyh_" + entry
    bad = [(dict(M=0), ESHAPE, b"M=0"), (dict(D=0), ESHAPE, b"D=0"), (dict(hidden=0), ESHAPE, b"hidden=0"),
           (dict(hidden=1025), ESHAPE, b"hidden=1025"), (dict(L=0), ESHAPE, b"layers"), (dict(L=17), ESHAPE, b"layers"),
           (dict(A=17), ESHAPE, b"A=17"), (dict(A=0), ESHAPE, b"A=0"), (dict(A=1, cont=0), ESHAPE, b"A=1"),
           (dict(A=13, actions=None), ESHAPE, b"packed records"), (dict(vmode=3), EINVAL, b"vloss_mode 3"),
           (dict(obs=None), EINVAL, b"null pointer"), (dict(rec=None), EINVAL, b"null pointer"), (dict(idx=None), EINVAL, b"null pointer"),
           (dict(params=None), EINVAL, b"null pointer"), (dict(offsets=None), EINVAL, b"null pointer"), (dict(grads=None), EINVAL, b"null pointer"),
           (dict(sc=None), EINVAL, b"null pointer"), (dict(ws=None), EINVAL, b"null pointer"),
           (dict(obs=_fake(4)), EINVAL, b"aligned"), (dict(rec=_fake(8)), EINVAL, b"aligned"), (dict(ws=_fake(16)), EINVAL, b"aligned"),
           (dict(offsets=outside), EINVAL, b"outside the bucket"), (dict(n_params=n_params - 1), EINVAL, b"outside the bucket")]
    if entry == "minibatch_f32":
        bad += [(dict(**{k: None}), EINVAL, b"null optimizer pointer") for k in ("m", "v", "lr", "t", "norm")]
    for over, rc, word in bad:
        got = call(name, **over)
        msg = lib.aurppo_last_error()
        assert got == rc and word in msg and name.encode() in msg, (list(over), got, msg)
        if "hidden" not in over and "offsets" not in over and "n_params" not in over:      # its sibling at 224: the same refusal
            offs_224, n_224 = _offsets(D_, 224, L, A_)
            assert call(SIBLINGS[name], **dict(dict(hidden=224, offsets=offs_224, n_params=n_224), **over)) == rc, list(over)
    assert call(SIBLINGS[name], hidden=200) == ESHAPE and b"hidden=200" in lib.aurppo_last_error()     # what the old entries still refuse
    assert call(SIBLINGS[name], hidden=48) == ESHAPE


def test_the_anyh_prepare_refuses_what_its_sibling_refuses(lib):
    p = _fake()
    L, D_, Hd, A_ = 2, 17, 200, 6
    offsets, n_params = _offsets(D_, Hd, L, A_)

    def call(name, **over):
        a = dict(dict(params=p, offsets=offsets, n_params=n_params, D=D_, hidden=Hd, L=L, wop=p), **over)
        off = (C.c_int * len(a["offsets"]))(*a["offsets"]) if a["offsets"] is not None else None
        return getattr(lib, name)(a["params"], off, a["n_params"], a["D"], a["hidden"], a["L"], a["wop"], None)
    outside = list(offsets)
    outside[2] = n_params - 8                      # the actor's second matrix
    name = "aurppo_mlp_layered_anyh_prep_f32"
    for over, rc, word in [(dict(D=0), ESHAPE, b"D=0"), (dict(hidden=0), ESHAPE, b"hidden=0"), (dict(hidden=1025), ESHAPE, b"hidden=1025"),
                           (dict(L=0), ESHAPE, b"layers"), (dict(L=17), ESHAPE, b"layers"),
                           (dict(params=None), EINVAL, b"null pointer"), (dict(offsets=None), EINVAL, b"null pointer"),
                           (dict(wop=None), EINVAL, b"null pointer"), (dict(wop=_fake(8)), EINVAL, b"aligned"),
                           (dict(offsets=outside), EINVAL, b"outside the bucket")]:
        got = call(name, **over)
        msg = lib.aurppo_last_error()
        assert got == rc and word in msg and name.encode() in msg, (list(over), got, msg)
    assert call("aurppo_mlp_layered_prep_f32") == ESHAPE and b"hidden=200" in lib.aurppo_last_error()
    assert call("aurppo_mlp_layered_prep_f32", hidden=48) == ESHAPE


# ------------------------------------------------------------------ (6) the per-product Python route refuses
def test_the_per_product_route_refuses_a_ragged_hidden_layout(monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    lay, bucket, obs, actions, rec, idx = _ragged(h, True, False)
    with pytest.raises(ValueError, match="mlp_layered_step_native"):
        H.mlp_layered_step(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF)
    hA, hC = h.t("hA", M, HIDDEN), h.t("hC", M, HIDDEN)
    with pytest.raises(ValueError, match="mlp_layered_step_native"):
        H.head_ppo(hA, hC, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF)
    with pytest.raises(ValueError, match="mlp_layered_step_native"):
        H.head_act(hA, hC, h.t("noise", M, A), bucket.flat_param, lay)
    assert h.calls == []                            # nothing reached the library


# ------------------------------------------------------------------ (7) the trainer's switch and its route choice
def _params(**over):
    p = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=3, gae=True, total_timesteps=48, anneal_lr=True, gae_lambda=0.95,
             num_update_epochs=1, num_envs=8, num_minibatches=2, entropy_coeff=0.0, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True,
             max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=200, continuous=True,
             learning_rate=3e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False, save=False,
             obs_dim=17, act_dim=3, device="cpu")
    p.update(over)
    return p


def _ops(**extra):
    ops = types.SimpleNamespace(**{k: getattr(oracle_ops, k) for k in dir(oracle_ops) if not k.startswith("__")})
    ops.mlp_layered_layout = H.mlp_layered_layout
    for k, v in extra.items():
        setattr(ops, k, v)
    return ops


def test_the_switch_is_off_by_default_and_passes_the_keyword_only_when_set(monkeypatch):
    from aur_ppo_amd import ppo as P
    assert P.LAYERED_ANY_HIDDEN_DEFAULT == "0"
    seen = []
    ops = types.SimpleNamespace(mlp_layered_layout=lambda policy, bucket, **kw: seen.append(kw))
    monkeypatch.delenv("AURPPO_LAYERED_ANY_HIDDEN", raising=False)
    P._layered_layout(ops, None, None)
    monkeypatch.setenv("AURPPO_LAYERED_ANY_HIDDEN", "0")
    P._layered_layout(ops, None, None)
    monkeypatch.setenv("AURPPO_LAYERED_ANY_HIDDEN", "1")
    P._layered_layout(ops, None, None)
    assert seen == [dict(any_state=True), dict(any_state=True), dict(any_state=True, any_hidden=True)]


def test_the_cpu_constructor_reads_no_layered_switch(monkeypatch):
    from aur_ppo_amd import ppo as P
    for k in ("AURPPO_LAYERED_STEP", "AURPPO_LAYERED_ACT", "AURPPO_LAYERED_ANY_HIDDEN"):
        monkeypatch.setenv(k, "1")
    a = P.ppo(_params(), ops=_ops())
    assert a._mlp is None and a._mlp_layered is None and a._mlp_layered_act is None and a._layered_native is False
    assert a._update_route(True) == "autograd"


def test_a_ragged_hidden_layout_takes_a_native_route_whatever_the_native_switch_says(monkeypatch):
    from aur_ppo_amd import ppo as P
    monkeypatch.delenv("AURPPO_LAYERED_NATIVE", raising=False)
    stub = lambda *a, **kw: None
    a = P.ppo(_params(), ops=_ops(mlp_layered_step=stub, mlp_layered_step_native=stub, mlp_layered_minibatch=stub))
    a._mlp_layered = H.mlp_layered_layout(a.policy, a.bucket, any_state=True, any_hidden=True)
    assert a._mlp_layered["ragged_hidden"] is True and a._layered_native is False
    assert a._update_route(True) in ("layered_minibatch", "layered_native_step")
    assert a._update_route(False) == "autograd"
    a._fused_adam = False                           # clip + Adam cannot ride along: the step alone, still native
    assert a._update_route(True) == "layered_native_step"
    # the aligned neighbour keeps the route it had: the per-product step until AURPPO_LAYERED_NATIVE says otherwise
    b = P.ppo(_params(hidden_dim=224), ops=_ops(mlp_layered_step=stub, mlp_layered_step_native=stub, mlp_layered_minibatch=stub))
    b._mlp_layered = H.mlp_layered_layout(b.policy, b.bucket, any_state=True, any_hidden=True)
    assert "ragged_hidden" not in b._mlp_layered and b._update_route(True) == "layered_step"


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
