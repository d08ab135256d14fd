"""CPU: the layered PPO step's shapes (tests/layered_cases.py).  (1) For every case of the GPU test, ANOTHER correct fp32
computation of the step -- ``ref64.make_alternative_fp32_net``: exact six-product matrix products, the kernels' tanh, a log-prob
with 1 / (std * std) formed once -- meets the same bars against the CPU yardstick: the bars the GPU test holds the kernels to can be
met at these shapes (the pattern of test_ref64_host.py::test_a_second_correct_fp32_formulation_meets_the_bars_of_every_class).
(2) Which policies ``hip_ops.mlp_layered_layout`` takes (it needs no device)."""
import pytest
import torch

from tests import layered_cases as LC
from tests import ref64 as R


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)       # fixed summation order in the CPU yardstick
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_a_second_correct_fp32_formulation_meets_the_bars_at_the_layered_shapes(c, one_thread):
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cpu")
    li = data["idx"].long()
    got = R.run_step(R.make_alternative_fp32_net(data["sd"]), data["obs"][li], data["act"][li] if c.cont else data["act"][li].long(),
                     data["rec"][li], R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
    R.check_step(c, got["scalars"], got["flat"], data["ref"], Y, Ys, "alternative fp32")


def _layouts(hidden, layers, D, A, cont=True):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    pol = actor_critic(D, (A,) if cont else A, hidden, layers, 0.0, cont)
    bucket = FlatBucket(pol.parameters())
    return H.mlp_layout(pol, bucket), H.mlp_layered_layout(pol, bucket)


@pytest.mark.parametrize("hidden,layers,D,A", [(64, 2, 64, 6), (128, 3, 128, 6)])
def test_the_fused_kernels_shapes_stay_with_them(hidden, layers, D, A):
    fused, layered = _layouts(hidden, layers, D, A)
    assert fused is not None and layered is None


@pytest.mark.parametrize("hidden,layers,D,A", [(100, 2, 144, 6), (256, 2, 20, 6), (256, 2, 64, 17), (1056, 2, 64, 6)])
def test_shapes_outside_the_layered_limits_are_refused(hidden, layers, D, A):
    fused, layered = _layouts(hidden, layers, D, A)
    assert fused is None and layered is None


@pytest.mark.parametrize("hidden,layers,D,A,cont", [(256, 2, 64, 6, True), (64, 2, 144, 6, True), (1024, 3, 256, 16, False)])
def test_wide_policies_get_a_layered_layout(hidden, layers, D, A, cont):
    from aur_ppo_amd import hip_ops as H
    fused, lay = _layouts(hidden, layers, D, A, cont)
    assert fused is None and isinstance(lay, dict)
    assert (lay["hidden"], lay["num_layers"], lay["D"], lay["A"], lay["continuous"]) == (hidden, layers, D, A, cont)
    assert len(lay["offsets"]) == 4 * (layers + 1) + 1 and len(H.head_layout(lay)) == 7
    n_w = sum((D * hidden + hidden) + (layers - 1) * (hidden * hidden + hidden) + (out * hidden + out) for out in (A, 1))
    assert lay["n_params"] == n_w + (A if cont else 0)


@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_every_case_is_a_layered_shape(c):
    fused, lay = _layouts(c.hidden, c.layers, c.D, c.A, c.cont)
    assert fused is None and lay is not None
