"""CPU: (1) the summation order of the bias gradient that k_linear_wgrad's BIAS builds take (csrc/linear_wgrad_body.h), emulated in
numpy, against the fp64 column sum; (2) which route ``ppo._update_route`` picks with and without ``AURPPO_LAYERED_NATIVE``.

(1) A workgroup's thread (row group g = 0..7, four columns) fetches rows ``g + 8 u + 32 c`` of its slice, u = 0..3 within chunk c, and
adds each dy value to its column's sum in that order; the eight row groups' sums are then added in group order and the slices' in slice
order.  The kernel keeps all three levels in fp64 and rounds to fp32 once.  Metric: ``|db - db64| / sum |dy|`` per column, the worst
column.  Y is CPU ``torch.sum`` in fp32 on the same metric, floored at 2^-24; the bar is ``ref64.MARGIN`` = 2: an fp64 accumulation
rounded once is bounded by 2^-24 |sum| <= 2^-24 sum |dy|, i.e. passes at <= 1, and 2 is the next power of two (DESIGN 2.2's argument
for ``norm``).  The same emulation with running fp32 sums per thread, row group and slice misses that bar in at least one draw: that is
what the bar is there to reject."""
import numpy as np
import pytest
import torch

from tests import ref64 as R
from tests import test_update_routes_host as UR

SIZES = [1, 31, 65, 257, 1000, 32785]
REGIMES = ["zero_mean", "offset"]
N_COLS, DRAWS = 8, 6


def _draw(M, regime, seed):
    rs = np.random.RandomState(seed)
    dy = rs.standard_normal((M, N_COLS)).astype(np.float32)
    if regime == "offset":
        dy += np.float32(3.0)
    return dy


def emulate(dy, rows_per_slice, acc):
    """The kernel's order with accumulators of dtype ``acc`` at every level; one rounding to fp32 at the end."""
    M = dy.shape[0]
    total = np.zeros(dy.shape[1], acc)
    for lo in range(0, M, rows_per_slice):
        hi = min(lo + rows_per_slice, M)
        groups = np.zeros((8, dy.shape[1]), acc)
        # rows g + 8 u + 32 c in (c, u) order are the rows lo + g, lo + g + 8, ... in ascending order: the eight groups step together
        for r in range(lo, hi, 8):
            blk = dy[r:min(r + 8, hi)]
            groups[:len(blk)] += blk.astype(acc)
        part = np.zeros(dy.shape[1], acc)
        for g in range(8):
            part += groups[g]
        total += part
    return total.astype(np.float32)


def _ratio(db, dy):
    d64 = dy.astype(np.float64)
    return float((np.abs(db.astype(np.float64) - d64.sum(0)) / np.abs(d64).sum(0)).max())


def _one_size(M, regime):
    """(worst fp64-order ratio to Y, worst fp32-running-sum ratio to Y) over the draws, one slice holding every row and 256-row slices."""
    worst64 = worst32 = 0.0
    for k in range(DRAWS):
        dy = _draw(M, regime, 1000 * M + k)
        Y = max(_ratio(torch.sum(torch.from_numpy(dy), 0).numpy(), dy), R.ULP32)
        for rps in {((M + 31) // 32) * 32, 256}:
            worst64 = max(worst64, _ratio(emulate(dy, rps, np.float64), dy) / Y)
            worst32 = max(worst32, _ratio(emulate(dy, rps, np.float32), dy) / Y)
    return worst64, worst32


_RESULTS = {}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M", SIZES)
def test_the_kernels_fp64_order_meets_the_bar(M, regime):
    w64, w32 = _RESULTS.setdefault((M, regime), _one_size(M, regime))
    print(f"\nM={M} {regime}: fp64 partials {w64:.2f} x Y, running fp32 sums {w32:.2f} x Y (bar {R.MARGIN:g})")
    assert w64 <= R.MARGIN


def test_running_fp32_sums_miss_the_bar_somewhere():
    worst = max(_RESULTS.setdefault((M, regime), _one_size(M, regime))[1] for M in SIZES for regime in REGIMES)
    print(f"\nrunning fp32 sums: worst {worst:.2f} x Y")
    assert worst > R.MARGIN


# ------------------------------------------------------------------ (2) the routes
class _NativeRecorder(UR.Recorder):
    """tests/test_update_routes_host.py's stand-in with the two native layered entry points."""

    def mlp_layered_step_native(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                                vloss_mode=1, out_scalars=None):
        self.log.append(("mlp_layered_step_native", self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef,
                                                                      vf_coef, norm_adv, vloss_mode, out_scalars)))
        return out_scalars

    def mlp_layered_minibatch(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                              out_scalars, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps, out_norm):
        e = self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars)
        self._adam(exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps)
        e.update(norm=self._row(out_norm, self._agent[0]._norms, 1))
        flat_grad.zero_()
        out_norm.zero_()
        self.log.append(("mlp_layered_minibatch", e))
        return out_scalars


def _native_agent(monkeypatch, rec64, native, dp=False, padded=False, fused_adam=True):
    monkeypatch.setattr(UR, "Recorder", _NativeRecorder)
    a, ops = UR._agent(monkeypatch, "layered", rec64)
    assert isinstance(ops, _NativeRecorder) and a._layered_native is False
    a._layered_native = native
    a._fused_adam = fused_adam
    if dp:
        a._dp = True
    if padded:
        a._mlp_layered = dict(a._mlp_layered, n_params=a._mlp_layered["n_params"] - 1)
    return a, ops


@pytest.mark.parametrize("rec64", [True, False])
def test_native_switch_single_process_takes_the_minibatch_call(monkeypatch, rec64):
    a, ops = _native_agent(monkeypatch, rec64, True)
    assert a._update_route(True) == "layered_minibatch"
    UR._run(a)
    pair = "packed" if rec64 else "separate"
    assert ops.log == [("mlp_layered_minibatch", dict(idx=UR._sl(s), pair=pair, scalars=k, layout="layered", norm=k))
                       for k, s in enumerate(UR.STEPS)]
    assert a.first_grad_probe == []          # nothing between the step and the optimizer to copy


@pytest.mark.parametrize("why", ["dp", "padded", "no_fused_adam"])
def test_native_switch_otherwise_takes_the_native_step_then_clip_and_adam(monkeypatch, why):
    a, ops = _native_agent(monkeypatch, True, True, dp=why == "dp", padded=why == "padded")
    if why == "no_fused_adam":
        a._fused_adam = False
        assert a._update_route(True) == "layered_native_step"
        return
    assert a._update_route(True) == "layered_native_step"
    UR._run(a)
    want = []
    for k, s in enumerate(UR.STEPS):
        want += [("mlp_layered_step_native", dict(idx=UR._sl(s), pair="packed", scalars=k, layout="layered")),
                 ("dist.allreduce_mean_", dict(world=1, force=why == "dp")),
                 ("clip_adam_", dict(norm=k, clip_n=None))]
    assert ops.log == want
    assert len(a.first_grad_probe) == 1 and bool((a.first_grad_probe[0] == 5.0).all())


def test_native_switch_without_the_entry_points_keeps_the_python_step(monkeypatch):
    a, _ops = UR._agent(monkeypatch, "layered", True)          # the plain stand-in: neither native attribute
    a._layered_native = True
    assert a._update_route(True) == "layered_step"


@pytest.mark.parametrize("route,want", [("chained", "chained"), ("halves_allreduce", "halves_allreduce"), ("halves_p2p", "halves_p2p"),
                                        ("fused", "fused_step"), ("layered", "layered_step"), ("autograd", "autograd")])
@pytest.mark.parametrize("env", [None, "0"])
def test_switch_unset_or_off_the_six_routes_are_chosen_as_before(monkeypatch, route, want, env):
    if env is None:
        monkeypatch.delenv("AURPPO_LAYERED_NATIVE", raising=False)
    else:
        monkeypatch.setenv("AURPPO_LAYERED_NATIVE", env)
    monkeypatch.setattr(UR, "Recorder", _NativeRecorder)       # the native attributes are there: only the switch keeps them unused
    a, _ops = UR._agent(monkeypatch, route, True)
    assert a._layered_native is False and a._update_route(True) == want
    assert a._update_route(False) == "autograd"
