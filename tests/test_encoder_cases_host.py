"""CPU: what the encoder's GPU suites rest on (tests/encoder_cases.py).
(1) The periodic and masked constructions of tests/test_encoder_large_gpu.py at a tiny size: the structured reference -- P base results,
    residue counts -- equals the direct fp64 result of the whole tensor to fp64 rounding.
(2) The host-side plans: for every K12 case of the edge and the large suites the library's own slice count (from
    aurppo_conv3x3_wgrad_ws_bytes, host code) equals the restated plan's, and the restated plan gives the slice length, last-slice
    length, chunk counts and kernel build each case's comment claims; for K11, NB and the buffer / 64-bit choice restate the two
    inequalities of aurppo_conv3x3_f32.
    What this does not see: the library exposes the slice COUNT alone.  Pixels per slice, the last slice's length and the chunk counts
    come from ``encoder_cases.k12_plan``, a transcription of conv_wgrad_plan; ``(S - 1) * pps < M <= S * pps`` with the library's S
    narrows a divergence of the two on the slice length and does not exclude it."""
import pytest
import torch

from tests import encoder_cases as E


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- (1)
def test_tiled_convolution_equals_the_base_images_convolutions():
    g = torch.Generator().manual_seed(1)
    P, B = 3, 8
    base = torch.randn(P, 2, 5, 4, generator=g, dtype=torch.float64)
    w = torch.randn(3, 2, 3, 3, generator=g, dtype=torch.float64)
    x = E.tile_images(base, B)
    assert all(torch.equal(x[b], base[b % P]) for b in range(B))
    direct, ref = E.conv64(x, w, 1), E.conv64(base, w, 1)
    assert E.compare_periodic(direct, ref, E.conv64(base.abs(), w.abs(), 1), images_per_chunk=4) <= 1e-15
    assert E.compare_periodic(E.dgrad64(x, w.transpose(0, 1).contiguous(), 1), E.dgrad64(base, w.transpose(0, 1).contiguous(), 1),
                              E.dgrad64(base.abs(), w.transpose(0, 1).abs().contiguous(), 1), images_per_chunk=7) <= 1e-15
    # the comparison sees one image from the wrong residue, and a NaN that was left
    wrong = direct.clone()
    wrong[7] = direct[6]
    assert E.compare_periodic(wrong, ref, E.conv64(base.abs(), w.abs(), 1), images_per_chunk=4) > 1e-3
    wrong = direct.clone()
    wrong[5, 1, 2, 3] = float("nan")
    assert E.compare_periodic(wrong, ref, E.conv64(base.abs(), w.abs(), 1), images_per_chunk=4) != \
        E.compare_periodic(wrong, ref, E.conv64(base.abs(), w.abs(), 1), images_per_chunk=4)       # NaN


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_masked_tiled_weight_gradient_equals_the_weighted_sum_of_base_gradients(pad):
    g = torch.Generator().manual_seed(2 + pad)
    P, B, Ci, Co, H, W = 3, 11, 2, 4, 5, 6
    base_x = torch.randn(P, Ci, H, W, generator=g)
    base_g = torch.randn(P, Co, H + 2 * pad - 2, W + 2 * pad - 2, generator=g)
    s = (torch.rand(B, generator=g) < 0.5).float()
    s[0], s[1] = 1.0, 0.0
    n = E.residue_counts(s, P)
    assert n.tolist() == [float(sum(s[b] for b in range(r, B, P))) for r in range(P)]
    x = E.tile_images(base_x, B)
    dy = E.tile_images(base_g, B) * s.view(-1, 1, 1, 1)
    direct, direct_mag = E.wgrad64(x, dy, Co, pad), E.wgrad64(x.abs(), dy.abs(), Co, pad)
    ref, mag = E.structured_wgrad64(base_x, base_g, s, Co, pad)
    assert float(((direct - ref).abs() / mag).max()) <= 1e-14
    assert float(((direct_mag - mag).abs() / mag).max()) <= 1e-14
    # an image taken from one place further on (another residue, another mask bit) is seen
    shifted = E.wgrad64(torch.roll(x, 1, 0), dy, Co, pad)
    assert float(((shifted - ref).abs() / mag).max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- (2)
LARGE_K12 = {        # shape -> (S, pixels per slice): tests/test_encoder_large_gpu.py
    (8800, 32, 64, 32, 32, 1): (252, 35776),
    (8800, 64, 64, 32, 32, 1): (168, 53664),
}


@pytest.mark.parametrize("shape", E.K12_SHAPES + list(LARGE_K12), ids=lambda s: "x".join(map(str, s)))
def test_k12_plans_are_what_the_cases_claim(lib, shape):
    B, Ci, Co, H, W, pad = shape
    plan = E.k12_plan(*shape)
    assert E.k12_slices_from_ws(lib.aurppo_conv3x3_wgrad_ws_bytes(*shape), Ci, Co) == plan["S"]
    assert plan["pps"] % 32 == 0 and (plan["S"] - 1) * plan["pps"] < plan["M"] <= plan["S"] * plan["pps"]
    if shape in E.K12_CLAIMS:
        S, pps, last, chunks, chunks_last, quad, WM = E.K12_CLAIMS[shape]
        assert (plan["S"], plan["pps"], plan["last"], plan["chunks"], plan["chunks_last"], plan["quad"], plan["WM"]) == \
            (S, pps, last, chunks, chunks_last, quad, WM)
    else:
        S, pps = LARGE_K12[shape]
        assert (plan["S"], plan["pps"]) == (S, pps) and plan["quad"]
        # the slices' first images: an early one's remaining bytes of dy are capped at 2^31, the last one's are not
        img = Co * plan["HoWo"] * 4
        b_last = (S - 1) * pps // plan["HoWo"]
        assert B * img > (1 << 31) and b_last * img > (1 << 31) and (B - b_last) * img < (1 << 31)
        assert pps % plan["HoWo"] != 0                       # slices begin inside images


def test_the_edge_cases_cover_the_chunk_counts_and_builds_of_k12():
    plans = [E.k12_plan(*s) for s in E.K12_SHAPES]
    single = [p for p in plans if p["S"] == 1]
    assert {p["chunks"] for p in single} >= {1, 2, 3}
    assert {(p["quad"], p["WM"]) for p in plans} == {(True, 1), (True, 2), (False, 1), (False, 2)}
    multi = [p for p in plans if p["S"] > 1]
    assert multi and all(p["last"] < p["pps"] and p["last"] % 32 != 0 and p["pps"] % p["HoWo"] != 0 for p in multi)
    assert {p["chunks"] % 2 for p in multi} == {0, 1} and all(p["chunks_last"] % 2 == 1 for p in multi)      # even and odd step counts
    assert all(s[1] * 9 % (64 * (4 // p["WM"])) != 0 for s, p in zip(E.K12_SHAPES, plans))      # Ci * 9 fills no column tile


def test_k11_plans_are_what_the_cases_claim():
    nbs = {E.k11_plan(B, ci, co, H, W)[0] for (B, ci, co, H, W, p) in E.K11_SHAPES}
    assert nbs == {1, 2, 4}
    assert all(E.k11_plan(B, ci, co, H, W)[1] for (B, ci, co, H, W, p) in E.K11_SHAPES)
    assert {B * (H + 2 * p - 2) * (W + 2 * p - 2) for (B, ci, co, H, W, p) in E.K11_SHAPES} >= {35, 256, 257, 300}
    # the large cases: 3 GiB is over 2^31 and takes the buffer build; 4 GiB + 4 MB does not
    assert E.k11_plan(12288, 16, 32, 64, 64) == (1, True) and 12288 * 16 * 64 * 64 * 4 == 3 << 30
    assert E.k11_plan(6144, 32, 16, 64, 64) == (1, True) and 6144 * 32 * 64 * 64 * 4 == 3 << 30
    assert E.k11_plan(4194304 + 4099, 16, 16, 4, 4) == (1, False)
    assert E.k11_plan((1 << 32) // 1024 - 1024, 16, 16, 4, 4) == (1, False) and E.k11_plan((1 << 32) // 1024 - 1025, 16, 16, 4, 4) == (1, True)


def test_guarded_views():
    for dtype in (torch.float32, torch.uint8):
        for aligned in (True, False):
            t = E.Guarded(3, 5, dtype=dtype, aligned=aligned, device="cpu")
            assert t.guards_intact() and not t.written()
            t.view.fill_(1)
            assert t.guards_intact() and t.written()
            t.buf[t.lo + t.n] = 0
            assert not t.guards_intact()
    w = E.Workspace(100, device="cpu")
    assert w.guards_intact() and w.view.numel() == 100
    w.buf[w.lo + 100] = 0
    assert not w.guards_intact()
