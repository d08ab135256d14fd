"""Cases of the layered PPO step and the layered rollout step at hidden widths that are no multiple of 32 (``mlp_layered_layout(...,
any_state=True, any_hidden=True)``: the policy runs at the width rounded up to 32 through the library's ``anyh`` entries,
csrc/layered.hip), shared by the GPU test (tests/test_layered_hidden_fp64_gpu.py) and the host test that shows the bars can be met at
these shapes (tests/test_layered_hidden_host.py).  A plain helper module: ``tests/ref64.py`` supplies the reference, the yardstick, the
metric and the bars, ``tests/layered_act_cases.py`` the rollout step's ``build`` / ``yardstick`` / ``metrics``, all unchanged.  Same
argument order as tests/layered_ragged_cases.py.

Hidden widths: 5 = one block of 32 columns, almost all of it pad; 33 = one column into a second block; 100 over a state of 376 floats =
D > hidden, a shape no native route took (K7w refuses the state, the layered routes refused the width); 129 and 130 = one and two columns
past a 128-column tile of the weight gradient, K13 / K14 at 160 padded columns (40 of a row's 64 threads hold columns); 200, 300, 400,
500 = the widths people type (400 / 300 is the classic continuous-control pair); 1000 = the last block of the largest shape (1024).  The
one-sample case is un-normalised (``norm_adv`` with M = 1 is NaN by construction)."""
from tests import ref64 as R

_mk = R._mk
STEP_CASES = [
    _mk("layered", 200, 2, 17, 6, True, 1000, True, 1),
    _mk("layered", 300, 2, 11, 3, True, 257, True, 1, "normal", "repeat", True),
    _mk("layered", 100, 1, 376, 16, True, 65, False, 0, "bf16half"),
    _mk("layered", 400, 3, 27, 8, True, 31, True, 2, "scaled", "perm", True),
    _mk("layered", 1000, 1, 3, 1, True, 2, False, 1),
    _mk("layered", 130, 2, 4, 2, False, 65, True, 1),
    _mk("layered", 200, 2, 8, 4, False, 1000, False, 0, "normal", "repeat"),
    _mk("layered", 33, 3, 129, 1, True, 1, False, 2),
    _mk("layered", 500, 2, 24, 4, True, 257, True, 1, "bf16half", "perm", True),
    _mk("layered", 5, 3, 129, 6, True, 1000, True, 0, "normal", "repeat"),
    _mk("layered", 129, 2, 64, 6, True, 257, True, 1),
]
STEP_IDS = [R.case_id(c) for c in STEP_CASES]
assert len(set(STEP_IDS)) == len(STEP_IDS)

# (hidden, layers, D, A, continuous, N, regime)
_ACT_SHAPES = [
    (200, 2, 17, 6, True, 257, "normal"),
    (300, 2, 11, 3, True, 1, "normal"),
    (100, 1, 376, 16, True, 65, "bf16half"),
    (130, 2, 4, 2, False, 255, "normal"),
    (1000, 1, 3, 1, True, 33, "scaled"),
    (400, 3, 27, 8, True, 1000, "normal"),
    (200, 2, 8, 4, False, 1000, "normal"),
    (33, 3, 129, 6, True, 257, "normal"),
    (5, 3, 129, 6, True, 257, "normal"),
]
ACT_CASES = [_mk("layered", h, l, D, A, cont, N, False, 0, regime) for h, l, D, A, cont, N, regime in _ACT_SHAPES]
ACT_IDS = [R.case_id(c) for c in ACT_CASES]
assert len(set(ACT_IDS)) == len(ACT_IDS)
