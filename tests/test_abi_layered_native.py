"""CPU: the native layered step at the ABI.  (1) The five prototypes parse out of include/aurppo.h and the bindings match them
(tests/test_abi_signatures.py covers every header symbol; here the five are named, with their shapes).  (2) The workspace plans and the
argument validation need no device.  (3) What ``linear_wgrad_bias``, ``mlp_layered_step_native`` and ``mlp_layered_minibatch`` hand to
the library at L = 1, 2, 3 over a state of 17 floats equals tests/transcripts/layered_native_calls.json (the recorder of
tests/test_hip_ops_calls.py, imported, as tests/test_layered_ragged_host.py uses it).

Re-record with ``python tests/test_abi_layered_native.py`` and READ THE DIFF whenever a C signature or a wrapper's argument list changes."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_abi_signatures as SIG           # noqa: E402
from tests import test_hip_ops_calls as TC             # noqa: E402
from tests import test_layered_ragged_host as RH       # noqa: E402

H = TC.H
TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "layered_native_calls.json")
NEW = {"aurppo_linear_wgrad_bias_ws_bytes": ("size_t", 3), "aurppo_linear_wgrad_bias_f32": ("int", 10),
       "aurppo_mlp_layered_step_workspace_bytes": ("size_t", 5), "aurppo_mlp_layered_step_f32": ("int", 22),
       "aurppo_mlp_layered_minibatch_f32": ("int", 31)}
EINVAL, ESHAPE = -1, -2


# ------------------------------------------------------------------ (1) prototypes and bindings
@pytest.mark.parametrize("name", sorted(NEW))
def test_the_prototype_parses_and_the_binding_matches(name):
    import __graft_entry__ as g
    g.build()
    res, types = SIG.PROTOTYPES[name]
    assert (res, len(types)) == NEW[name]
    fn = getattr(TC._lib.load(), name)
    assert len(fn.argtypes) == len(types) and all(SIG._matches(t, d) for t, d in zip(fn.argtypes, types))
    assert fn.restype is (C.c_size_t if res == "size_t" else C.c_int)


def test_the_step_follows_the_wide_steps_argument_order():
    """aurppo_mlp_wide_ppo_step_f32 without its two event handles; aurppo_mlp_wide_ppo_minibatch_f32 without next_idx, next_M, chained."""
    P = SIG.PROTOTYPES
    assert P["aurppo_mlp_layered_step_f32"][1] == P["aurppo_mlp_wide_ppo_step_f32"][1][:-2]
    wide = P["aurppo_mlp_wide_ppo_minibatch_f32"][1]
    assert P["aurppo_mlp_layered_minibatch_f32"][1] == wide[:-5] + wide[-2:]
    rows = P["aurppo_linear_wgrad_rows_f32"][1]
    assert P["aurppo_linear_wgrad_bias_f32"][1] == rows[:4] + ["float*"] + rows[4:]


# ------------------------------------------------------------------ (2) plans and validation without a device
def test_workspace_plans_and_refusals_without_gpu():
    import __graft_entry__ as g
    g.build()
    lib = TC._lib.load()
    for M, N, K in [(1, 32, 16), (257, 256, 17), (131072, 256, 256), (131072, 1024, 376)]:
        plain, bias = lib.aurppo_linear_wgrad_ws_bytes(M, N, K), lib.aurppo_linear_wgrad_bias_ws_bytes(M, N, K)
        assert bias >= plain + 8 * N and (bias - plain) % (8 * N) <= 16, (M, N, K, plain, bias)      # S x N doubles behind the products
    assert lib.aurppo_linear_wgrad_bias_ws_bytes(0, 32, 16) == 0 and lib.aurppo_linear_wgrad_bias_ws_bytes(4, 0, 16) == 0
    for M, D, A, Hd, L in [(1, 144, 6, 64, 1), (257, 17, 6, 256, 2), (131072, 64, 6, 256, 3), (131072, 376, 16, 1024, 16)]:
        nb = lib.aurppo_mlp_layered_step_workspace_bytes(M, D, A, Hd, L)
        parts = (2 * L * M * Hd * 4 + lib.aurppo_conv3x3_wop_bytes(max(D, Hd), Hd)
                 + max(lib.aurppo_linear_wgrad_bias_ws_bytes(M, Hd, D), lib.aurppo_linear_wgrad_bias_ws_bytes(M, Hd, Hd))
                 + lib.aurppo_head_ppo_workspace_bytes(M, Hd, A) + lib.aurppo_clip_workspace_bytes(1))
        assert parts <= nb <= parts + 5 * 128, (M, D, A, Hd, L, nb, parts)
    assert lib.aurppo_mlp_layered_step_workspace_bytes(131072, 376, 16, 1024, 16) > 1 << 32          # computed and returned in size_t
    for M, D, A, Hd, L in [(0, 64, 6, 256, 2), (4, 0, 6, 256, 2), (4, 64, 17, 256, 2), (4, 64, 0, 256, 2), (4, 64, 6, 48, 2),
                           (4, 64, 6, 1056, 2), (4, 64, 6, 256, 0), (4, 64, 6, 256, 17)]:
        assert lib.aurppo_mlp_layered_step_workspace_bytes(M, D, A, Hd, L) == 0, (M, D, A, Hd, L)
    # null pointers are refused before anything else is looked at; a shape outside the limits before any launch
    assert lib.aurppo_mlp_layered_step_f32(*([None] * 4), 4, 64, 6, 1, 256, 2, None, None, 0, None, 0.2, 0.01, 0.5, 1, 1, None, None, None) == EINVAL
    assert b"null pointer" in lib.aurppo_last_error()
    assert lib.aurppo_linear_wgrad_bias_f32(*([None] * 5), 4, 32, 16, None, None) == EINVAL
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.aurppo_linear_wgrad_bias_f32(p, p, None, p, p, 4, 32, 17, p, None) == ESHAPE       # no index, K no multiple of 4
    assert b"multiple of 4" in lib.aurppo_last_error()


# ------------------------------------------------------------------ (3) what the host layer hands to the library
CASES = {}
M = TC.M


def _wgrad_bias_case(with_rows):
    def run(h):
        gy, x = h.t("gy", M, 32), h.t("x", TC.B, 17) if with_rows else h.t("x", M, 20)
        dw, db = H.linear_wgrad_bias(gy, x, h.idx("rows") if with_rows else None)
        assert dw.shape == (32, x.shape[1]) and db.shape == (32,)
        h.name("dw", dw), h.name("db", db)
    return run


def _native_case(layers, cont, packed, minibatch):
    def run(h):
        lay, bucket, obs, actions, rec, idx = RH._ragged(h, layers, cont, packed)
        sc = h.t("scalars", 9)
        knobs = (TC.CLIP, TC.ENT, TC.VF, True, H.VLOSS_OLDVALUES)
        if minibatch:
            m, v, lr, step, norms = TC._adam(h, bucket)
            assert H.mlp_layered_minibatch(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, *knobs, sc, m, v, lr, step,
                                           TC.MAX_NORM, TC.BETAS, TC.EPS, norms[1:2]) is sc
        else:
            assert H.mlp_layered_step_native(obs, actions, rec, idx, bucket.flat_param, lay, bucket.flat_grad, *knobs, sc) is sc
    return run


CASES["linear_wgrad_bias/plain"] = _wgrad_bias_case(False)
CASES["linear_wgrad_bias/rows/K17"] = _wgrad_bias_case(True)
CASES["mlp_layered_step_native/D17/L1/continuous/packed"] = _native_case(1, True, True, False)
CASES["mlp_layered_step_native/D17/L2/continuous"] = _native_case(2, True, False, False)
CASES["mlp_layered_step_native/D17/L3/categorical"] = _native_case(3, False, False, False)
CASES["mlp_layered_minibatch/D17/L1/categorical"] = _native_case(1, False, False, True)
CASES["mlp_layered_minibatch/D17/L2/continuous/packed"] = _native_case(2, True, True, True)
CASES["mlp_layered_minibatch/D17/L3/continuous"] = _native_case(3, True, False, True)


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


def test_one_library_call_per_step_with_the_layout_as_it_is():
    """One size request, one workspace, one call; the state width 17, the layer count and the 4 (L + 1) + 1 offsets reach the library."""
    rec = _recorded()
    for L, name in [(1, "mlp_layered_step_native/D17/L1/continuous/packed"), (3, "mlp_layered_step_native/D17/L3/categorical"),
                    (2, "mlp_layered_minibatch/D17/L2/continuous/packed")]:
        fns = [fn for fn, _ in rec[name]]
        entry = "aurppo_mlp_layered_minibatch_f32" if "minibatch" in name else "aurppo_mlp_layered_step_f32"
        assert fns == ["aurppo_mlp_layered_step_workspace_bytes", "_workspace", entry], fns
        args = rec[name][2][1]
        assert args[4:10] == [M, 17, TC.A, int("categorical" not in name), RH.HIDDEN, L] and len(args[11]) == 4 * (L + 1) + 1
        assert rec[name][0][1] == [M, 17, TC.A, RH.HIDDEN, L] and rec[name][1][1][0] == "layered_step"
        assert (args[1] is None) == ("packed" in name) and args[-2] == "ws:layered_step+0" and args[-1] == "stream"


def test_every_call_fits_the_bound_argtypes(monkeypatch):
    """The same cases against the real binding's ``argtypes`` (count and ctypes conversion; nothing is launched)."""
    import __graft_entry__ as g
    g.build()
    bound = TC._lib.load()
    for name in sorted(CASES):
        with monkeypatch.context() as m:
            assert run_case(name, m.setattr, bound)


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
