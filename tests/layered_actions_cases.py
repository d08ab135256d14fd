"""Cases of the layered PPO step at action heads of 17 .. 32 outputs (``mlp_layered_layout(..., wide_actions=True)``: the library's ``wa``
entries, K13 / K14's builds with 32-long per-action arrays, csrc/head.hip), shared by the GPU test (tests/test_layered_actions_fp64_gpu.py)
and the host test that shows the bars can be met at these shapes (tests/test_layered_actions_host.py).  A plain helper module:
``tests/ref64.py`` supplies the reference, the yardstick, the metric and the bars, all unchanged.  Same argument order as
tests/layered_hidden_cases.py.

Action counts: 17 = the first past the old limit (Humanoid: 376 state floats, 2 x 256), 20 and 24 = the dexterous hands' range, 31 and 32 = the
last slots of the 32-long arrays.  Hidden widths: 32 (8 threads per row, 32 row groups per workgroup), 64, 96 (32 threads per row, 24 of
them with columns), 160, 256, 512, 1024 (four waves per row; 33 x 1024 floats of head weights in LDS, the largest shape), 200 (a ragged
hidden width: the head rows in the bucket are shorter than the LDS rows).  A Gaussian head with more than 12 actions has no packed records;
the Categorical heads take them.  The one-sample case is un-normalised (``norm_adv`` with M = 1 is NaN by construction)."""
from tests import ref64 as R

_mk = R._mk
STEP_CASES = [
    _mk("layered", 256, 2, 376, 17, True, 1000, True, 1),                                # Humanoid
    _mk("layered", 256, 2, 64, 17, True, 1, False, 0),
    _mk("layered", 160, 1, 16, 32, True, 31, True, 2, "scaled", "repeat"),
    _mk("layered", 1024, 1, 64, 32, True, 257, True, 1, "bf16half"),                     # the LDS extreme, 4 waves per row
    _mk("layered", 64, 2, 144, 24, True, 65, False, 1),
    _mk("layered", 512, 3, 144, 17, False, 257, True, 1, "normal", "perm", True),        # Categorical, packed records
    _mk("layered", 1024, 2, 16, 32, False, 1000, False, 0, "normal", "repeat"),
    _mk("layered", 160, 2, 64, 32, False, 2, True, 1),
    _mk("layered", 256, 2, 17, 31, True, 257, True, 2, "scaled"),                        # ragged state
    _mk("layered", 200, 2, 17, 17, True, 257, True, 1),                                  # ragged hidden: Hr != H
    _mk("layered", 96, 1, 144, 20, False, 65, True, 1),                                  # TPR 32 with idle lanes (H / 4 = 24)
    _mk("layered", 32, 1, 144, 32, True, 1000, True, 1),                                 # TPR 8: 32 row groups per workgroup
]
STEP_IDS = [R.case_id(c) for c in STEP_CASES]
assert len(set(STEP_IDS)) == len(STEP_IDS)
