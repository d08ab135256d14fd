"""GPU: aurppo_linear_wgrad_bias_f32 alone -- k_linear_wgrad's BIAS builds (csrc/linear_wgrad_body.h), which leave the layer's bias
gradient, the column sums of dy, beside the weight gradient.

Per shape and addressing (plain, a permutation, a repeating index): x lies inside a NaN-filled buffer and every row the index does not
name is NaN; dw and db are views with 64 floats of NaN either side.  dw equals the call without the bias output bit for bit; db sits
within ``ref64.MARGIN`` x Y of the fp64 column sum on the scale sum |dy|, Y being ``torch.sum`` in fp32 on the GPU on the same metric,
floored at 2^-24 (an fp64 accumulation rounded once is bounded by 2^-24 |sum| <= 2^-24 sum |dy|); a second launch gives the same
bits; an all-zero dy gives db == 0.  Without an index a K that is no multiple of 4 is AURPPO_ESHAPE: that build does not exist."""
import ctypes as C

import pytest
import torch

from tests import ref64 as R
from tests import test_linear_ragged_gpu as LRG

pytestmark = pytest.mark.gpu

ESHAPE = -2
# (M, N, K): one row; a ragged K under one chunk; two chunks, two tiles either way; several slices; N off the tile, K = 100;
# many slices over a K of three tiles
SHAPES = [(1, 32, 16), (31, 32, 17), (33, 160, 160), (257, 256, 64), (1000, 132, 100), (4097, 64, 376)]
KINDS = ["plain", "perm", "repeat"]
WORST = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _operands(M, N, K, kind, g):
    if kind == "plain":
        rows, B = None, M
        _buf, x = LRG._guarded_x(B, K, torch.arange(M, device="cuda", dtype=torch.int32), g)
    else:
        B = M + 37
        rows = LRG._index(M, B, kind, g)
        rows[M // 2] = B - 1                 # the last row of x is named
        _buf, x = LRG._guarded_x(B, K, rows, g)
    # an offset regime in the odd columns: the sums there are of the order of M, the rounding of a running fp32 sum with them
    dy = torch.randn(M, N, device="cuda", generator=g)
    dy[:, 1::2] += 3.0
    return _buf, x, rows, dy


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bias_build_under_guards(M, N, K, kind):
    from aur_ppo_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M + N + K + len(kind))
    _buf, x, rows, dy = _operands(M, N, K, kind, g)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.aurppo_linear_wgrad_bias_ws_bytes(M, N, K), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= lib.aurppo_linear_wgrad_ws_bytes(M, N, K)
    if rows is None and K % 4 != 0:
        dw, db = LRG._Guarded(N, K), LRG._Guarded(N)
        rc = lib.aurppo_linear_wgrad_bias_f32(_p(dy), _p(x), None, _p(dw.view), _p(db.view), M, N, K, _p(ws), st)
        torch.cuda.synchronize()
        assert rc == ESHAPE and dw.guards_intact() and db.guards_intact()
        assert bool(torch.isnan(dw.view).all()) and bool(torch.isnan(db.view).all()), "refused before any launch"
        return
    ref = LRG._Guarded(N, K)
    assert lib.aurppo_linear_wgrad_rows_f32(_p(dy), _p(x), _p(rows), _p(ref.view), M, N, K, _p(ws), st) == 0
    runs = []
    for _ in range(2):
        dw, db = LRG._Guarded(N, K), LRG._Guarded(N)
        ws.fill_(0xFF)                       # NaN in every float and double of the workspace
        rc = lib.aurppo_linear_wgrad_bias_f32(_p(dy), _p(x), _p(rows), _p(dw.view), _p(db.view), M, N, K, _p(ws), st)
        torch.cuda.synchronize()
        assert rc == 0 and dw.guards_intact() and db.guards_intact()
        runs.append((dw.view.clone(), db.view.clone()))
    (dw1, db1), (dw2, db2) = runs
    assert bool(torch.isfinite(dw1).all()) and bool(torch.isfinite(db1).all())
    assert torch.equal(dw1, ref.view), "dw differs from the call without the bias output"
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2), "two launches differ"
    db64 = dy.double().sum(0)
    scale = dy.double().abs().sum(0)
    err = ((db1.double() - db64).abs() / scale).max().item()
    Y = max(((torch.sum(dy, 0).double() - db64).abs() / scale).max().item(), R.ULP32)
    WORST[(M, N, K, kind)] = err / Y
    print(f"\n[wgrad bias] M={M} N={N} K={K} {kind}: {err:.3e} = {err / Y:.2f} x Y (Y {Y:.3e}); worst so far {max(WORST.values()):.2f} x Y")
    assert err <= R.MARGIN * Y, (err, Y, err / Y)


@pytest.mark.parametrize("M,N,K,kind", [(257, 256, 64, "plain"), (1000, 132, 100, "perm"), (31, 32, 17, "repeat")])
def test_all_zero_dy_gives_zero(M, N, K, kind):
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M + 37, K, device="cuda", generator=g)
    rows = None if kind == "plain" else LRG._index(M, M + 37, kind, g)
    dw, db = H.linear_wgrad_bias(torch.zeros(M, N, device="cuda"), x[:M].contiguous() if rows is None else x, rows)
    assert dw.shape == (N, K) and db.shape == (N,)
    assert bool((db == 0).all()) and bool((dw == 0).all())
