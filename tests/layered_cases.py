"""Cases of the layered PPO step (hip_ops.mlp_layered_step: the MLP shapes wider than the fused kernels) shared by the GPU test
(tests/test_layered_fp64_gpu.py) and the host test that shows the bars can be met at these shapes (tests/test_layered_host.py).
A plain helper module: ``tests/ref64.py`` supplies the reference, the yardstick, the metric and the bars, unchanged.

What the list covers: hidden 64 (over D = 144), 160, 256, 512, 1024; one to three layers; D in {16, 64, 144, 256}; Gaussian heads of
1, 6, 12, 16 actions and Categorical heads of 2 and 16; M in {1, 2, 31, 65, 257, 1000} and once 32 768 + 17; the three value modes,
both normalisations, ``perm`` and ``repeat`` indices, packed and unpacked records, the three observation regimes.  The seeds are
``ref64._mk``'s own: the host emulation (whose 1 / (std * std) shortcut sits near the scalar bar, tests/test_layered_host.py) meets
the bars with them (worst gradient 0.87 x Y of 2, worst scalar 10.8 x Y of 16)."""
from tests import ref64 as R

_mk = R._mk
CASES = [
    _mk("layered", 256, 2, 64, 6, True, 1000, True, 1),
    _mk("layered", 256, 2, 64, 6, True, 32768 + 17, True, 1, "normal", "repeat", True),
    _mk("layered", 64, 2, 144, 6, True, 257, True, 1, "bf16half"),
    _mk("layered", 64, 1, 144, 1, True, 1, False, 0),
    _mk("layered", 160, 3, 144, 12, True, 65, False, 2, "scaled", "repeat", True),
    _mk("layered", 160, 1, 16, 2, False, 2, True, 1),
    _mk("layered", 512, 3, 144, 16, True, 31, True, 0),
    _mk("layered", 512, 2, 256, 16, False, 257, True, 1, "bf16half", "perm", True),
    _mk("layered", 1024, 1, 64, 6, True, 65, False, 1, "scaled"),
    _mk("layered", 1024, 3, 256, 12, True, 1000, True, 2, "normal", "perm", True),
    _mk("layered", 1024, 2, 16, 2, False, 1000, False, 0, "normal", "repeat"),
    _mk("layered", 256, 3, 256, 1, True, 31, True, 2, "bf16half", "repeat"),
    _mk("layered", 256, 1, 16, 16, False, 65, True, 2, "scaled", "perm", True),
    _mk("layered", 160, 2, 64, 6, True, 1000, False, 1),
    _mk("layered", 512, 1, 16, 6, True, 2, False, 1),
    _mk("layered", 64, 3, 144, 2, False, 1000, True, 1, "normal", "repeat"),
    _mk("layered", 256, 2, 144, 12, True, 257, False, 0, "scaled", "perm", True),
    _mk("layered", 512, 2, 64, 1, True, 1000, True, 1, "normal", "perm", True),
    _mk("layered", 1024, 2, 144, 16, True, 257, True, 1, "bf16half"),
    _mk("layered", 160, 3, 256, 6, True, 1000, True, 0, "normal", "repeat"),
]
IDS = [R.case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)
