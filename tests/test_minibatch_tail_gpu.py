"""GPU: the per-minibatch tail behind K7 (k_mlp_step3) -- the gradient slabs, their fixed-order reduce and the optimizer launch
that refreshes K7's operand copies.

(a) With static tiles (AURPPO_STATIC_TILES=1) the gradient must equal, bit for bit, a float32 numpy replay of k_mlp_reduce's
    tree over the slabs read back from the workspace: rows grouped b = grp (mod 16), ((x0 + x4) + x8) + x12 per quarter,
    (a0 + a1) + (a2 + a3), the 16 groups folded 0 -> 15 from 0; and the rest of what the reduce writes must equal its numpy
    replay too: the nine loss scalars folded from the per-slab loss partials (lane l adds rows l, l + 64, ... in double, then
    the 64-lane shuffle-down tree), and, for a whole minibatch, the clip's partial sums of squares (one per 64 parameters).
(b) After a chained minibatch the bf16-plane operand copies (wop3) that the optimizer launch left must equal, element for
    element and padding included, the image that the non-chained entry builds from the updated parameters (bf16x3.h
    wop3_prepare, run by k_adv_stats_idx; k_mlp3_prep's launch before).
Both run at D in {64, 17}, continuous and discrete heads, M in {131072, 16384}, with the shuffle pipeline on a side stream
meanwhile, as in test_determinism.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B_SHUF = 524288
K_MAX_GRID, K_STAT_BLOCKS = 256, 256
WOP3_BYTES = 2 * 4 * 3 * 4 * 3 * 64 * 8          # bf16x3.h kWopElems: 4 roles x 3 matrices x 4 k-steps x 3 planes x 512


def _r64(x):
    return (x + 63) // 64 * 64


def slab_stride(n_params):
    """mlp_common.h slab_stride: slab b's parameter p sits at float b * slab_stride + p."""
    return _r64(n_params)


def ws_layout(n_params):
    """Byte offsets of mlp.hip's workspace carve-up (ws_view)."""
    loss_part = 8 * 2 * K_STAT_BLOCKS
    slabs = loss_part + 8 * 8 * K_MAX_GRID
    stamps = _r64(slabs + 4 * K_MAX_GRID * slab_stride(n_params))
    w1op = stamps + 8 * 44 * K_MAX_GRID
    tile_counter = w1op + 4 * 4 * 32 * 64
    sq_part = tile_counter + 4 * 16
    wop3 = sq_part + _r64(8 * ((n_params + 63) // 64))
    return dict(loss_part=loss_part, slabs=slabs, sq_part=sq_part, wop3=wop3)


def k7_grid(M):
    """mlp.hip mlp_step_impl: how many K7 workgroups (= slabs) a launch at minibatch M uses."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    spare = int(os.environ.get("AURPPO_MLP_SPARE_CUS", "8") or 8)
    spare = spare if spare >= 0 else 8
    grid = max(1, min(cus - spare, K_MAX_GRID))
    n_tiles = (M + 31) // 32
    if 2 * grid < n_tiles <= 2 * cus and cus <= K_MAX_GRID:
        grid = cus
    return min(grid, (n_tiles + 1) // 2)


def replay_reduce(slabs):
    """k_mlp_reduce's tree in float32, per parameter, over (n_slabs, n_params) slabs."""
    n_slabs, n = slabs.shape
    zero = np.zeros(n, np.float32)
    t = np.zeros(n, np.float32)
    for grp in range(16):
        x = [slabs[grp + 16 * j] if grp + 16 * j < n_slabs else zero for j in range(16)]
        a4 = [((x[k] + x[k + 4]) + x[k + 8]) + x[k + 12] for k in range(4)]
        t = t + ((a4[0] + a4[1]) + (a4[2] + a4[3]))
    return t


def wave_sum(v):
    """common.h wave_sum over 64 lanes (lane 0's value): v[l] += v[l + off] for off = 32, 16, ..., 1, in double."""
    v = np.asarray(v, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:off] + v[off:2 * off]
    return v[0]


def replay_scalars(loss_part, n_slabs, M, ent_coef, vf_coef):
    """The reduce's loss-scalar fold over (n_slabs, 8) double partials -> the nine float32 scalars (include/aurppo.h order)."""
    r = []
    for q in range(6):
        lanes = np.zeros(64, np.float64)
        for l in range(64):
            s = 0.0
            for b in range(l, n_slabs, 64):
                s = s + loss_part[b, q]
            lanes[l] = s
        r.append(wave_sum(lanes))
    f = np.float32
    pg, vl, ent = f(r[0] / M), f(0.5) * f(r[1] / M), f(r[2] / M)
    loss = (pg - f(ent_coef) * ent) + vl * f(vf_coef)
    return np.array([loss, pg, vl, ent, f(r[3] / M), f(r[4] / M), f(r[5] / M), f(loss_part[0, 6]), f(loss_part[0, 7])], np.float32)


def replay_sq_part(grads):
    """The clip's partial sums: per 64 consecutive parameters, wave_sum of (double) g * (double) g, lane = p mod 64."""
    n = grads.size
    g = np.zeros((n + 63) // 64 * 64, np.float64)
    g[:n] = grads.astype(np.float64)
    return np.array([wave_sum(blk * blk) for blk in g.reshape(-1, 64)])


def side_shuffle(H):
    """Start the shuffle pipeline (fill / accept / link / resolve) on a side stream behind what the main stream has queued."""
    rng = H.MT19937(1, B_SHUF, torch.device("cuda"))
    side = torch.cuda.Stream()
    perm_out = torch.empty((4, B_SHUF), dtype=torch.int32, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rng.shuffle_epochs(B_SHUF, 4, out=perm_out)
    return rng, perm_out


def _setup(D, A, cont, B=262144, seed=0):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(D, (A,) if cont else A, 64, 2, 0.0, cont).cuda()
    with torch.no_grad():
        if cont:
            pol.actor_logstd.copy_(0.3 * torch.randn(1, A))
        for p in pol.parameters():
            p.add_((0.05 if cont else 0.3) * torch.randn_like(p))
    bucket = FlatBucket(pol.parameters())
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn(B, D, device="cuda", generator=g)
    act = (torch.randn(B, A, device="cuda", generator=g) if cont
           else torch.randint(0, A, (B,), device="cuda", generator=g).float())
    with torch.no_grad():
        _, lp, _, v = pol.evaluate(obs, act)
    rec = torch.stack([lp + 0.2 * torch.randn(B, device="cuda", generator=g), 2 * torch.randn(B, device="cuda", generator=g),
                       v.view(-1) + torch.randn(B, device="cuda", generator=g),
                       v.view(-1) + 0.1 * torch.randn(B, device="cuda", generator=g)], 1).contiguous()
    return H, pol, bucket, obs, act, rec


CASES = [(D, cont, M) for D in (64, 17) for cont in (True, False) for M in (131072, 16384)]


@pytest.mark.parametrize("D,cont,M", CASES, ids=[f"D{D}-{'cont' if c else 'disc'}-M{M}" for D, c, M in CASES])
def test_gradient_is_the_fixed_tree_over_the_slabs(D, cont, M, monkeypatch):
    monkeypatch.setenv("AURPPO_STATIC_TILES", "1")
    monkeypatch.setenv("AURPPO_K7_VARIANT", "3")
    A = 6 if cont else 4
    H, pol, bucket, obs, act, rec = _setup(D, A, cont)
    lay = H.mlp_layout(pol, bucket)
    assert lay is not None and not lay.get("wide")
    n = lay["n_params"]
    idx = torch.randperm(obs.shape[0], device="cuda")[:M].int()
    keep = side_shuffle(H)
    g = torch.full_like(bucket.flat_grad, float("nan"))
    sc = H.mlp_ppo_step(obs, act, rec, idx, bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1)
    torch.cuda.synchronize()
    ws = H._ws_cache[("mlp", torch.cuda.current_device())]
    off = ws_layout(n)
    grid = k7_grid(M)
    ns = slab_stride(n)
    slabs = ws[off["slabs"]:off["slabs"] + 4 * grid * ns].view(torch.float32).view(grid, ns)[:, :n].cpu().numpy()
    assert np.isfinite(slabs).all()
    want = replay_reduce(slabs)
    got = g[:n].cpu().numpy()
    bad = np.flatnonzero(want.view(np.uint32) != got.view(np.uint32))
    print(f"D={D} cont={cont} M={M}: grid {grid}, n_params {n}, mismatching gradient elements {bad.size}")
    assert bad.size == 0, (bad[:8], want[bad[:8]], got[bad[:8]])
    lp = ws[off["loss_part"]:off["loss_part"] + 8 * 8 * grid].view(torch.float64).view(grid, 8).cpu().numpy()
    want_sc = replay_scalars(lp, grid, M, 0.01, 0.5)
    got_sc = sc.cpu().numpy()
    print(f"  loss scalars {got_sc.tolist()}, replay {want_sc.tolist()}")
    assert np.array_equal(want_sc.view(np.uint32), got_sc.view(np.uint32)), (want_sc, got_sc)
    # a whole minibatch on a copy of the weights: the same slabs (static tiles, K7 reads the weights before the optimizer launch),
    # and the reduce now also leaves the clip's partial sums
    dev = torch.device("cuda")
    p2 = bucket.flat_param.clone()
    g2 = torch.empty_like(bucket.flat_grad)
    m_, v_ = torch.zeros_like(p2), torch.zeros_like(p2)
    sc2, norm = torch.empty(9, device=dev), torch.empty(1, device=dev)
    keep2 = side_shuffle(H)
    H.mlp_ppo_minibatch(obs, act, rec, idx, p2, lay, g2, 0.2, 0.01, 0.5, True, 1, sc2, m_, v_, torch.tensor([3e-4], device=dev),
                        torch.zeros(1, device=dev), 0.5, (0.9, 0.999), 1e-5, norm)
    torch.cuda.synchronize()
    n_red = (n + 63) // 64
    got_sq = ws[off["sq_part"]:off["sq_part"] + 8 * n_red].view(torch.float64).cpu().numpy()
    want_sq = replay_sq_part(want)
    bad_sq = np.flatnonzero(want_sq.view(np.uint64) != got_sq.view(np.uint64))
    print(f"  clip partial sums differing from the replay {bad_sq.size} of {n_red}")
    assert bad_sq.size == 0, (bad_sq[:8], want_sq[bad_sq[:8]], got_sq[bad_sq[:8]])
    assert np.array_equal(want_sc.view(np.uint32), sc2.cpu().numpy().view(np.uint32))
    del keep, keep2


@pytest.mark.parametrize("D,cont,M", CASES, ids=[f"D{D}-{'cont' if c else 'disc'}-M{M}" for D, c, M in CASES])
def test_chained_operand_copies_match_a_fresh_prepare(D, cont, M, monkeypatch):
    monkeypatch.setenv("AURPPO_K7_VARIANT", "3")
    A = 6 if cont else 4
    H, pol, bucket, obs, act, rec = _setup(D, A, cont)
    lay = H.mlp_layout(pol, bucket)
    n = lay["n_params"]
    perm = torch.randperm(obs.shape[0], device="cuda").int()
    idx0, idx1 = perm[:M], perm[M:2 * M]
    dev = torch.device("cuda")
    m_, v_ = torch.zeros_like(bucket.flat_param), torch.zeros_like(bucket.flat_param)
    lr, step = torch.tensor([3e-4], device=dev), torch.zeros(1, device=dev)
    sc, norm = torch.empty(9, device=dev), torch.empty(1, device=dev)
    keep = side_shuffle(H)
    for k, (i, nxt) in enumerate(((idx0, idx1), (idx1, None))):
        H.mlp_ppo_minibatch(obs, act, rec, i, bucket.flat_param, lay, bucket.flat_grad, 0.2, 0.01, 0.5, True, 1, sc, m_, v_, lr,
                            step, 0.5, (0.9, 0.999), 1e-5, norm, next_idx=nxt, chained=k == 1)
    torch.cuda.synchronize()
    ws = H._ws_cache[("mlp", torch.cuda.current_device())]
    o = ws_layout(n)["wop3"]
    chained = ws[o:o + WOP3_BYTES].clone()
    # the non-chained entry rebuilds the copies from the (updated) parameters (k_adv_stats_idx) before its K7 launch
    g = torch.empty_like(bucket.flat_grad)
    H.mlp_ppo_step(obs, act, rec, idx0, bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1)
    torch.cuda.synchronize()
    fresh = ws[o:o + WOP3_BYTES].clone()
    a, b = chained.view(torch.int16).cpu().numpy(), fresh.view(torch.int16).cpu().numpy()
    bad = np.flatnonzero(a != b)
    print(f"D={D} cont={cont} M={M}: wop3 elements differing from a fresh prepare {bad.size} of {a.size}")
    assert float(step) == 2.0
    assert bad.size == 0, bad[:8]
    del keep
