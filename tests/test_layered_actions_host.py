"""CPU: the layered routes at action heads of 17 .. 32 outputs (tests/layered_actions_cases.py).  (1) For every case of the GPU test,
ANOTHER correct fp32 computation -- ``ref64.make_alternative_fp32_net`` -- meets the same bars against the CPU yardstick: the bars the
GPU test holds the kernels to can be met at these shapes without exclusions.  (2) Which policies ``hip_ops.mlp_layered_layout`` takes with
``wide_actions=True`` and which it still refuses (it needs no device).  (3) What ``head_ppo``, ``head_act``, ``mlp_layered_step_native``,
``mlp_layered_minibatch``, ``mlp_layered_prepare`` and ``mlp_layered_act`` (unpaired, paired, value-only) hand to the library at 17 actions
equals tests/transcripts/layered_actions_calls.json (the recorder of tests/test_hip_ops_calls.py, imported): the ``wa`` entries with the
siblings' arguments, and the ``anyh`` entries for what does not depend on the action count.  (4) The size functions.  (5) Every ``wa``
entry refuses what lies outside 1 .. 32 (Categorical 2 .. 32) and a packed Gaussian head of 17, with nothing launched.  (6) The per-product
Python route refuses a wide-action layout.  (7) The trainer's switch and its route choice.

Re-record with ``python tests/test_layered_actions_host.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
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

from tests import layered_actions_cases as LW          # noqa: E402
from tests import oracle_ops                           # noqa: E402
from tests import ref64 as R                           # noqa: E402
from tests import test_abi_signatures as SIG           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_actions_calls.json")
N, A, D, HIDDEN, LAYERS = 4, 17, 24, 160, 2
M, B = TC.M, TC.B
EINVAL, ESHAPE = -1, -2
SIBLINGS = {"aurppo_head_ppo_wa_workspace_bytes": "aurppo_head_ppo_workspace_bytes", "aurppo_head_ppo_wa_f32": "aurppo_head_ppo_f32",
            "aurppo_head_act_wa_f32": "aurppo_head_act_f32"}
SIBLINGS.update({"aurppo_mlp_layered_wa_" + n: "aurppo_mlp_layered_anyh_" + n
                 for n in ("step_workspace_bytes", "step_f32", "minibatch_f32", "act_f32", "act_paired_f32")})


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
@pytest.mark.parametrize("c", LW.STEP_CASES, ids=LW.STEP_IDS)
def test_a_second_correct_fp32_formulation_meets_the_bars_at_the_wide_action_step_shapes(c, one_thread):
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cpu")
    li = data["idx"].long()
    got = R.run_step(R.make_alternative_fp32_net(data["sd"]), data["obs"][li], data["act"][li] if c.cont else data["act"][li].long(),
                     data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    R.check_step(c, got["scalars"], got["flat"], data["ref"], Y, Ys, "alternative fp32")


# ------------------------------------------------------------------ (2) the layout rule
def _layouts(hidden, layers, D_, A_, cont=True, **kw):
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(D_, (A_,) if cont else A_, hidden, layers, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    return H.mlp_layout(pol, bucket), H.mlp_layered_layout(pol, bucket, **kw)


@pytest.mark.parametrize("hidden,layers,D_,A_,cont", [(256, 2, 376, 17, True), (160, 1, 16, 32, True), (512, 3, 144, 17, False),
                                                      (1024, 2, 16, 32, False)])
def test_wide_actions_gives_17_to_32_actions_a_layered_layout_of_the_unpadded_policy(hidden, layers, D_, A_, cont):
    fused, lay = _layouts(hidden, layers, D_, A_, cont, any_state=True, wide_actions=True)
    assert fused is None and isinstance(lay, dict) and lay["layered"] is True and lay["wide_actions"] is True and "ragged_hidden" not in lay
    assert (lay["hidden"], lay["num_layers"], lay["D"], lay["A"], lay["continuous"]) == (hidden, layers, D_, A_, cont)
    assert len(lay["offsets"]) == 4 * (layers + 1) + 1 and len(H.head_layout(lay)) == 7
    n_w = sum((D_ * hidden + hidden) + (layers - 1) * (hidden * hidden + hidden) + (out * hidden + out) for out in (A_, 1))
    assert lay["n_params"] == n_w + (A_ if cont else 0)         # nothing of the 32-long arrays is in the bucket
    # without the keyword these stay refused
    assert _layouts(hidden, layers, D_, A_, cont, any_state=True)[1] is None
    assert _layouts(hidden, layers, D_, A_, cont, any_state=True, any_hidden=True)[1] is None
    assert _layouts(hidden, layers, D_, A_, cont, any_state=True, wide_actions=False)[1] is None


def test_33_actions_get_no_layout_either_way():
    for cont in (True, False):
        assert _layouts(256, 2, 16, 33, cont, any_state=True, any_hidden=True, wide_actions=True) == (None, None)
        assert _layouts(256, 2, 16, 33, cont, any_state=True)[1] is None
    assert H.MLP_LAYERED_MAX_A == 32 and H.MLP_MAX_A == 16


def test_16_actions_or_fewer_keep_their_layout_under_wide_actions():
    for A_ in (6, 16):
        _fused, lay = _layouts(256, 2, 17, A_, any_state=True, wide_actions=True)
        assert lay is not None and "wide_actions" not in lay
        assert lay == _layouts(256, 2, 17, A_, any_state=True)[1]


def test_the_state_and_hidden_rules_follow_their_own_keywords():
    assert _layouts(256, 2, 17, 17, wide_actions=True)[1] is None                          # a ragged state still needs any_state
    assert _layouts(200, 2, 16, 17, wide_actions=True)[1] is None                          # a ragged hidden width still needs any_hidden
    both = _layouts(200, 2, 17, 17, any_state=True, any_hidden=True, wide_actions=True)[1]
    assert both["wide_actions"] is True and both["ragged_hidden"] is True
    assert _layouts(1056, 2, 16, 17, any_hidden=True, wide_actions=True)[1] is None


@pytest.mark.parametrize("hidden,layers,D_", [(64, 2, 64), (100, 2, 17), (128, 3, 128)])
def test_the_fused_kernels_shapes_stay_refused_at_17_actions_by_both_layouts(hidden, layers, D_):
    """K7 / K7w's action width is theirs (AP = 16): a shape they would take but for its 17 actions gets no layout of either kind."""
    assert _layouts(hidden, layers, D_, 17, any_state=True, any_hidden=True, wide_actions=True) == (None, None)
    assert _layouts(hidden, layers, D_, 17) == (None, None)
    fused, layered = _layouts(hidden, layers, D_, 16, any_state=True, any_hidden=True, wide_actions=True)
    assert fused is not None and layered is None


@pytest.mark.parametrize("c", LW.STEP_CASES, ids=LW.STEP_IDS)
def test_every_case_is_a_wide_action_layered_shape(c):
    fused, lay = _layouts(c.hidden, c.layers, c.D, c.A, c.cont, any_state=True, any_hidden=True, wide_actions=True)
    assert fused is None and lay is not None and lay["wide_actions"] is True and 17 <= c.A <= 32
    assert _layouts(c.hidden, c.layers, c.D, c.A, c.cont, any_state=True, any_hidden=True)[1] is None
    assert not (c.packed and c.cont)                    # 17 action floats do not fit a packed record


# ------------------------------------------------------------------ (3) what the host layer hands to the library at 17 actions
CASES = {}


def _wide(h, cont, packed):
    """(layout, bucket, obs, actions, rec, idx) of a 2 x 160 policy with 17 actions over 24 state floats, its layout through ``wide_actions``."""
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(D, (A,) if cont else A, HIDDEN, LAYERS, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    h.name("param", bucket.flat_param)
    h.name("grad", bucket.flat_grad)
    assert H.mlp_layered_layout(pol, bucket, any_state=True) is None
    lay = H.mlp_layered_layout(pol, bucket, any_state=True, wide_actions=True)
    assert lay["A"] == A and lay["wide_actions"] and "ragged_hidden" not in lay and lay["offsets"][2] != 0 and lay["continuous"] == cont
    obs = h.t("obs", B, D)
    if packed:
        actions, rec = None, h.t("rec64", B, 16)
    else:
        actions, rec = (h.t("actions", B, A) if cont else h.t("actions", B)), h.t("rec", B, 4)
    return lay, bucket, obs, actions, rec, h.idx("idx")


def _step_case(cont, packed, minibatch):
    def run(h):
        lay, bucket, obs, actions, rec, idx = _wide(h, cont, packed)
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
        lay, bucket, *_ = _wide(h, cont, False)
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


def _head_case(cont, packed, act):
    def run(h):
        lay, bucket, _obs, actions, rec, idx = _wide(h, cont, packed)
        hA, hC = h.t("hA", N if act else M, HIDDEN), h.t("hC", N if act else M, HIDDEN)
        if act:
            nz = h.t("noise", N, A) if cont else h.t("noise", N)
            assert H.head_act(hA, hC, nz, bucket.flat_param, lay, *_outs(h, cont))[2].shape == (N,)
        else:
            sc = h.t("scalars", 9)
            assert H.head_ppo(hA, hC, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True, H.VLOSS_CLIPPED,
                              sc) is sc
    return run


CASES["mlp_layered_step_native/A17/continuous"] = _step_case(True, False, False)
CASES["mlp_layered_step_native/A17/categorical/packed"] = _step_case(False, True, False)
CASES["mlp_layered_minibatch/A17/continuous"] = _step_case(True, False, True)
CASES["mlp_layered_act/A17/continuous/prepared"] = _act_case(True, "prepared", False)
CASES["mlp_layered_act/A17/categorical/prepared/paired"] = _act_case(False, "prepared", True)
CASES["mlp_layered_act/A17/continuous/value_only"] = _act_case(True, "value_only", False)
CASES["head_ppo/A17/continuous"] = _head_case(True, False, False)
CASES["head_ppo/A17/categorical/packed"] = _head_case(False, True, False)
CASES["head_act/A17/continuous"] = _head_case(True, False, True)


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


def test_the_entries_are_the_wa_ones_and_the_anyh_ones_where_the_action_count_does_not_matter():
    """Every library call of every case is a ``wa`` entry -- or, for the operand copies and the rollout workspace, an ``anyh`` one --
    ``A`` arrives as 17, and the layered workspaces are keyed apart from the 16-action ones."""
    where = {"aurppo_mlp_layered_wa_step_workspace_bytes": 2, "aurppo_mlp_layered_wa_step_f32": 6, "aurppo_mlp_layered_wa_minibatch_f32": 6,
             "aurppo_mlp_layered_wa_act_f32": 4, "aurppo_mlp_layered_wa_act_paired_f32": 4, "aurppo_head_ppo_wa_workspace_bytes": 2,
             "aurppo_head_ppo_wa_f32": 9, "aurppo_head_act_wa_f32": 5}
    no_a = {"aurppo_mlp_layered_anyh_wop_bytes", "aurppo_mlp_layered_anyh_prep_f32", "aurppo_mlp_layered_anyh_act_workspace_bytes"}
    seen = set()
    for name, calls in _recorded().items():
        for fn, args in calls:
            if fn == "_workspace":
                assert args[0] in ("layered_step_wa", "layered_act_wa", "head"), (name, args)
                continue
            assert fn in where or fn in no_a, (name, fn)
            if fn in where:
                assert args[where[fn]] == A, (name, fn, args)
            seen.add(fn)
    assert seen == set(where) | no_a


def test_a_wa_call_differs_from_its_sibling_in_the_entry_and_the_workspace_key_alone(monkeypatch):
    """A 16-action policy's layout with and without ``wide_actions``: same arguments in the same order, call for call."""
    def calls(wide):
        h = TC.Harness()
        h.install(monkeypatch.setattr)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        H._layered_wop_cache.clear()
        from aur_ppo_amd.actor_critic import actor_critic
        from aur_ppo_amd.flat import FlatBucket
        pol = actor_critic(D, (16,), HIDDEN, LAYERS, 0.0, True)
        bucket = FlatBucket(pol.parameters())
        h.name("param", bucket.flat_param)
        h.name("grad", bucket.flat_grad)
        lay = H.mlp_layered_layout(pol, bucket, any_state=True, wide_actions=True)
        assert "wide_actions" not in lay
        if wide:
            lay["wide_actions"] = True
        obs, actions, rec, idx = h.t("obs", B, D), h.t("actions", B, 16), h.t("rec", B, 4), h.idx("idx")
        H.mlp_layered_step_native(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF, True,
                                  H.VLOSS_CLIPPED, h.t("scalars", 9))
        H.mlp_layered_act(h.t("obs4", N, D), h.t("noise", N, 16), bucket.flat_param, lay, h.t("actions_out", N, 16), h.t("logp", N),
                          h.t("value", N), paired=True)
        H.head_ppo(h.t("hA", M, HIDDEN), h.t("hC", M, HIDDEN), actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF)
        for key, wop in H._layered_wop_cache.items():
            h.name("wop", wop)
        H._layered_wop_cache.clear()
        return json.loads(json.dumps(h.transcript()))
    on, off = calls(True), calls(False)
    assert len(on) == len(off) > 0
    plain = {"aurppo_mlp_layered_anyh_" + n: "aurppo_mlp_layered_" + n for n in ("wop_bytes", "prep_f32", "act_workspace_bytes", "step_f32",
                                                                                "step_workspace_bytes", "act_paired_f32")}
    for (fa, aa), (fb, ab) in zip(on, off):
        if fa == "_workspace":
            assert fb == "_workspace" and aa[0] in (ab[0] + "_wa", "head") and aa[1] == ab[1]
        else:
            sib = SIBLINGS.get(fa, fa)
            assert plain.get(sib, sib) == fb, (fa, fb)
            assert [str(x).replace("_wa", "") for x in aa] == [str(x) for x in ab], (fa, aa, ab)


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
def test_the_size_functions_take_up_to_32_actions_and_equal_the_siblings_up_to_16(lib):
    for Hd, L, D_ in ((256, 2, 376), (200, 1, 17), (1024, 3, 16), (32, 1, 144)):
        Hp = (Hd + 31) // 32 * 32
        for M_ in (1, 257, 131072):
            for A_ in (1, 6, 16):
                assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(M_, D_, A_, Hd, L) == lib.aurppo_mlp_layered_anyh_step_workspace_bytes(M_, D_, A_, Hd, L) > 0
                assert lib.aurppo_head_ppo_wa_workspace_bytes(M_, Hp, A_) == lib.aurppo_head_ppo_workspace_bytes(M_, Hp, A_) > 0
            at16 = lib.aurppo_mlp_layered_wa_step_workspace_bytes(M_, D_, 16, Hd, L), lib.aurppo_head_ppo_wa_workspace_bytes(M_, Hp, 16)
            for A_ in (17, 32):
                assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(M_, D_, A_, Hd, L) > at16[0]
                assert lib.aurppo_head_ppo_wa_workspace_bytes(M_, Hp, A_) > at16[1]
                assert lib.aurppo_mlp_layered_anyh_step_workspace_bytes(M_, D_, A_, Hd, L) == 0 and lib.aurppo_head_ppo_workspace_bytes(M_, Hp, A_) == 0
            for A_ in (0, 33, -1):
                assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(M_, D_, A_, Hd, L) == 0 and lib.aurppo_head_ppo_wa_workspace_bytes(M_, Hp, A_) == 0
    # what else the siblings' size functions refuse
    assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(0, 17, 17, 256, 2) == 0 and lib.aurppo_mlp_layered_wa_step_workspace_bytes(65, 0, 17, 256, 2) == 0
    assert lib.aurppo_mlp_layered_wa_step_workspace_bytes(65, 17, 17, 1025, 2) == 0 and lib.aurppo_mlp_layered_wa_step_workspace_bytes(65, 17, 17, 256, 17) == 0
    assert lib.aurppo_head_ppo_wa_workspace_bytes(0, 256, 17) == 0 and lib.aurppo_head_ppo_wa_workspace_bytes(65, 200, 17) == 0
    assert lib.aurppo_head_ppo_wa_workspace_bytes(65, 1056, 17) == 0


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


def _refused(lib, name, got, rc, word):
    msg = lib.aurppo_last_error()
    assert got == rc and word in msg and name.encode() in msg, (name, got, msg)


@pytest.mark.parametrize("entry", ["act_f32", "act_paired_f32"])
def test_the_wa_act_refuses_outside_its_limits(entry, lib):
    p = _fake()
    L, D_, Hd = 2, 64, 200
    name = "aurppo_mlp_layered_wa_" + entry

    def call(fn, A_, cont=1, **over):
        offsets, n_params = _offsets(D_, Hd, L, max(A_, 1))
        a = dict(dict(obs=p, noise=p, N=4, D=D_, hidden=Hd, L=L, params=p, n_params=n_params, actions=p, logp=p, value=p, wop=p, ws=p), **over)
        off = (C.c_int * len(offsets))(*offsets)
        return getattr(lib, fn)(a["obs"], a["noise"], a["N"], a["D"], A_, cont, a["hidden"], a["L"], a["params"], off, a["n_params"],
                                a["actions"], a["logp"], a["value"], a["wop"], a["ws"], None)
    for A_, cont, word in [(33, 1, b"A=33"), (0, 1, b"A=0"), (1, 0, b"A=1"), (33, 0, b"A=33"), (-1, 1, b"A=-1")]:
        _refused(lib, name, call(name, A_, cont), ESHAPE, word)
        assert b"1..32" in lib.aurppo_last_error()
    for over, rc, word in [(dict(N=0), ESHAPE, b"N=0"), (dict(hidden=1025), ESHAPE, b"hidden=1025"), (dict(L=17), ESHAPE, b"layers"),
                           (dict(obs=None), EINVAL, b"null pointer"), (dict(actions=None), EINVAL, b"null pointer"),
                           (dict(ws=_fake(16)), EINVAL, b"aligned"), (dict(n_params=100), EINVAL, b"outside the bucket")]:
        _refused(lib, name, call(name, 17, **over), rc, word)
    # the siblings keep their limit and their words
    sib = SIBLINGS[name]
    _refused(lib, sib, call(sib, 17), ESHAPE, b"A=17 (1..16, Categorical: 2..16)")


@pytest.mark.parametrize("entry", ["step_f32", "minibatch_f32"])
def test_the_wa_step_refuses_outside_its_limits(entry, lib):
    p = _fake()
    L, D_, Hd = 2, 17, 200
    name = "aurppo_mlp_layered_wa_" + entry

    def call(fn, A_, cont=1, **over):
        offsets, n_params = _offsets(D_, Hd, L, max(A_, 1))
        a = dict(dict(obs=p, actions=p, rec=p, idx=p, M=4, D=D_, hidden=Hd, L=L, params=p, n_params=n_params, grads=p, vmode=1, sc=p, m=p, v=p,
                      lr=p, t=p, norm=p, ws=p), **over)
        off = (C.c_int * len(offsets))(*offsets)
        args = [a["obs"], a["actions"], a["rec"], a["idx"], a["M"], a["D"], A_, cont, a["hidden"], a["L"], a["params"], off, a["n_params"],
                a["grads"], 0.2, 0.01, 0.5, 1, a["vmode"], a["sc"]]
        if fn.endswith("minibatch_f32"):
            args += [a["m"], a["v"], 0.5, a["lr"], a["t"], 0.9, 0.999, 1e-5, a["norm"]]
        return getattr(lib, fn)(*args, a["ws"], None)
    for A_, cont, word in [(33, 1, b"A=33"), (0, 1, b"A=0"), (1, 0, b"A=1"), (33, 0, b"A=33")]:
        _refused(lib, name, call(name, A_, cont), ESHAPE, word)
        assert b"1..32" in lib.aurppo_last_error()
    for A_ in (13, 17, 32):                             # a Gaussian head of more than 12 actions needs `actions`
        _refused(lib, name, call(name, A_, actions=None), ESHAPE, b"packed records")
        assert f"A={A_}".encode() in lib.aurppo_last_error()
    for over, rc, word in [(dict(M=0), ESHAPE, b"M=0"), (dict(hidden=1025), ESHAPE, b"hidden=1025"), (dict(L=0), ESHAPE, b"layers"),
                           (dict(vmode=3), EINVAL, b"vloss_mode 3"), (dict(rec=None), EINVAL, b"null pointer"),
                           (dict(rec=_fake(8)), EINVAL, b"aligned"), (dict(n_params=100), EINVAL, b"outside the bucket")]:
        _refused(lib, name, call(name, 17, **over), rc, word)
    if entry == "minibatch_f32":
        _refused(lib, name, call(name, 17, m=None), EINVAL, b"null optimizer pointer")
    sib = SIBLINGS[name]
    _refused(lib, sib, call(sib, 17), ESHAPE, b"A=17 (1..16, Categorical: 2..16)")


def test_the_wa_head_entries_refuse_outside_their_limits(lib):
    p = _fake()
    Hd = 256

    def ppo_(fn, A_, cont=1, **over):
        a = dict(dict(hA=p, hC=p, gzA=p, gzC=p, actions=p, rec=p, idx=p, M=4, H=Hd, params=p, n_params=40 * Hd, grads=p, sc=p, ws=p), **over)
        lay = (C.c_int * 7)(0, 33 * Hd, 34 * Hd, 35 * Hd, 36 * Hd, 37 * Hd, 38 * Hd)
        return getattr(lib, fn)(a["hA"], a["hC"], a["gzA"], a["gzC"], a["actions"], a["rec"], a["idx"], a["M"], a["H"], A_, cont, a["params"],
                                lay, a["n_params"], a["grads"], 0.2, 0.01, 0.5, 1, 1, a["sc"], a["ws"], None)

    def act_(fn, A_, cont=1, **over):
        a = dict(dict(hA=p, hC=p, noise=p, N=4, H=Hd, params=p, n_params=40 * Hd, actions=p, logp=p, value=p), **over)
        lay = (C.c_int * 5)(0, 33 * Hd, 34 * Hd, 35 * Hd, 36 * Hd)
        return getattr(lib, fn)(a["hA"], a["hC"], a["noise"], a["N"], a["H"], A_, cont, a["params"], lay, a["n_params"], a["actions"],
                                a["logp"], a["value"], None)
    for call, name in ((ppo_, "aurppo_head_ppo_wa_f32"), (act_, "aurppo_head_act_wa_f32")):
        for A_, cont, word in [(33, 1, b"A=33"), (0, 1, b"A=0"), (1, 0, b"A=1"), (33, 0, b"A=33")]:
            _refused(lib, name, call(name, A_, cont), ESHAPE, word)
            assert b"1..32" in lib.aurppo_last_error()
        _refused(lib, name, call(name, 17, H=200), ESHAPE, b"H=200")
        _refused(lib, name, call(name, 17, H=1056), ESHAPE, b"H=1056")
        _refused(lib, name, call(name, 17, hC=None), EINVAL, b"null pointer")
        _refused(lib, name, call(name, 17, n_params=100), EINVAL, b"outside the bucket")
        _refused(lib, SIBLINGS[name], call(SIBLINGS[name], 17), ESHAPE, b"A=17 (1..16, Categorical: 2..16)")
    for A_ in (13, 17, 32):
        _refused(lib, "aurppo_head_ppo_wa_f32", ppo_("aurppo_head_ppo_wa_f32", A_, actions=None), ESHAPE, b"packed records")
        assert f"A={A_}".encode() in lib.aurppo_last_error()
    _refused(lib, "aurppo_head_ppo_wa_f32", ppo_("aurppo_head_ppo_wa_f32", 17, M=0), ESHAPE, b"M=0")
    _refused(lib, "aurppo_head_act_wa_f32", act_("aurppo_head_act_wa_f32", 17, N=0), ESHAPE, b"N=0")


# ------------------------------------------------------------------ (6) the per-product Python route refuses
def test_the_per_product_route_refuses_a_wide_action_layout(monkeypatch):
    h = TC.Harness()
    h.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    lay, bucket, obs, actions, rec, idx = _wide(h, True, False)
    with pytest.raises(ValueError, match="mlp_layered_step_native"):
        H.mlp_layered_step(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF)
    assert h.calls == []                            # nothing reached the library
    # 17 Gaussian action floats do not fit a packed record: the wrappers say so before the library is reached
    with pytest.raises(ValueError, match="buffer shapes"):
        H.mlp_layered_step_native(obs, None, h.t("rec64", B, 16), idx, bucket.flat_param, lay, bucket.flat_grad, TC.CLIP, TC.ENT, TC.VF)
    assert h.calls == []


# ------------------------------------------------------------------ (7) the trainer's switch and its route choice
def _params(**over):
    p = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=3, gae=True, total_timesteps=48, anneal_lr=True, gae_lambda=0.95,
             num_update_epochs=1, num_envs=8, num_minibatches=2, entropy_coeff=0.0, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True,
             max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=256, continuous=True,
             learning_rate=3e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False, save=False,
             obs_dim=24, act_dim=17, device="cpu")
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
    assert P.LAYERED_WIDE_ACTIONS_DEFAULT == "0"
    seen = []
    ops = types.SimpleNamespace(mlp_layered_layout=lambda policy, bucket, **kw: seen.append(kw))
    monkeypatch.delenv("AURPPO_LAYERED_ANY_HIDDEN", raising=False)
    monkeypatch.delenv("AURPPO_LAYERED_WIDE_ACTIONS", raising=False)
    P._layered_layout(ops, None, None)
    monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "0")
    P._layered_layout(ops, None, None)
    monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "1")
    P._layered_layout(ops, None, None)
    monkeypatch.setenv("AURPPO_LAYERED_ANY_HIDDEN", "1")
    P._layered_layout(ops, None, None)
    assert seen == [dict(any_state=True), dict(any_state=True), dict(any_state=True, wide_actions=True),
                    dict(any_state=True, any_hidden=True, wide_actions=True)]


def test_a_17_action_policy_takes_a_native_route_with_the_switch_and_autograd_without(monkeypatch):
    from aur_ppo_amd import ppo as P
    monkeypatch.delenv("AURPPO_LAYERED_NATIVE", raising=False)
    monkeypatch.delenv("AURPPO_LAYERED_ANY_HIDDEN", raising=False)
    stub = lambda *a, **kw: None
    ops = _ops(mlp_layered_step=stub, mlp_layered_step_native=stub, mlp_layered_minibatch=stub)
    a = P.ppo(_params(), ops=ops)
    assert a._mlp is None and a._mlp_layered is None and a._update_route(True) == "autograd"        # (the CPU constructor reads no switch)
    monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "1")
    a._mlp_layered = P._layered_layout(ops, a.policy, a.bucket)
    assert a._mlp_layered["wide_actions"] is True and a._mlp_layered["A"] == 17 and a._layered_native is False
    assert a._update_route(True) in ("layered_minibatch", "layered_native_step")
    assert a._update_route(False) == "autograd"
    a._fused_adam = False                           # clip + Adam cannot ride along: the step alone, still native, never the per-product one
    assert a._update_route(True) == "layered_native_step"
    assert a._step_pair()[0] is not None            # 17 action floats: the actions beside (B, 4) records, never packed ones
    # with the switch off the same policy has no layered layout: autograd
    monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "0")
    a._mlp_layered = P._layered_layout(ops, a.policy, a.bucket)
    assert a._mlp_layered is None and a._update_route(True) == "autograd"
    # 16 actions keep the route they had: the per-product step until AURPPO_LAYERED_NATIVE says otherwise
    monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "1")
    b = P.ppo(_params(act_dim=16), ops=ops)
    b._mlp_layered = P._layered_layout(ops, b.policy, b.bucket)
    assert "wide_actions" not in b._mlp_layered and b._update_route(True) == "layered_step"


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
