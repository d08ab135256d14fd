"""Cases of the layered PPO step and the layered rollout step at state widths that are no multiple of 16 (``mlp_layered_layout(...,
any_state=True)``: layer 0's products on the tail builds k_linear_tail / k_linear_wgrad_tail of csrc/linear.hip), shared by the GPU test
(tests/test_layered_ragged_fp64_gpu.py) and the host test that shows the bars can be met at these shapes
(tests/test_layered_ragged_host.py).  A plain helper module: ``tests/ref64.py`` supplies the reference, the yardstick, the metric and the
bars, ``tests/layered_act_cases.py`` the rollout step's ``build`` / ``yardstick`` / ``metrics``, all unchanged.

State widths: the environments the reference's CLI is used with -- Pendulum 3, CartPole 4, LunarLander 8, Hopper 11, HalfCheetah 17,
BipedalWalker 24, Ant 27, Humanoid 376 -- and 1 and 129.  For the kernels: 1, 3, 4, 8, 11 = a single k-step whose tail sits in the
first or the second lane half; 17 = a k-step plus a column with rows off 16-byte alignment; 24, 27 = a second k-step that ends in its
first / second lane half; 129 = a staged chunk boundary plus a column and a second 128-column tile of the weight gradient; 376 = a tail
of exactly one lane half, D > hidden.  The one-sample case is un-normalised (``norm_adv`` with M = 1 is NaN by construction)."""
from tests import ref64 as R

_mk = R._mk
STEP_CASES = [
    _mk("layered", 256, 2, 17, 6, True, 1000, True, 1),
    _mk("layered", 256, 2, 11, 3, True, 257, True, 1, "normal", "repeat", True),
    _mk("layered", 64, 1, 376, 16, True, 65, False, 0, "bf16half"),
    _mk("layered", 512, 3, 27, 8, True, 31, True, 2, "scaled", "perm", True),
    _mk("layered", 1024, 1, 3, 1, True, 2, False, 1),
    _mk("layered", 160, 2, 4, 2, False, 65, True, 1),
    _mk("layered", 256, 2, 8, 4, False, 1000, False, 0, "normal", "repeat"),
    _mk("layered", 256, 3, 1, 1, True, 1, False, 2),
    _mk("layered", 512, 2, 24, 4, True, 257, True, 1, "bf16half", "perm", True),
    _mk("layered", 160, 3, 129, 6, True, 1000, True, 0, "normal", "repeat"),
]
STEP_IDS = [R.case_id(c) for c in STEP_CASES]
assert len(set(STEP_IDS)) == len(STEP_IDS)

# (hidden, layers, D, A, continuous, N, regime)
_ACT_SHAPES = [
    (256, 2, 17, 6, True, 257, "normal"),
    (256, 2, 11, 3, True, 1, "normal"),
    (64, 1, 376, 16, True, 65, "bf16half"),
    (160, 2, 4, 2, False, 255, "normal"),
    (1024, 1, 3, 1, True, 33, "scaled"),
    (512, 3, 27, 8, True, 1000, "normal"),
    (256, 2, 8, 4, False, 1000, "normal"),
    (160, 3, 129, 6, True, 257, "normal"),
]
ACT_CASES = [_mk("layered", h, l, D, A, cont, N, False, 0, regime) for h, l, D, A, cont, N, regime in _ACT_SHAPES]
ACT_IDS = [R.case_id(c) for c in ACT_CASES]
assert len(set(ACT_IDS)) == len(ACT_IDS)
