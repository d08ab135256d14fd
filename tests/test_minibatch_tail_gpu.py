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
Both run at D in {64, 17}, continuous and discrete heads, M in {131072, 16384} and, over a smaller buffer, M in {33, 1071, 8200}
(1, 17 and 129 slabs: one slab row, one group boundary crossed, half the groups with a ninth row), with the shuffle pipeline on a side
stream meanwhile, as in test_determinism.py.  Every bucket here is 1 or 3 (D = 17 with three actions) past a multiple of 4, so
k_mlp_reduce_x4's guarded last quad runs.
(c) K7w (mlp_wide.hip) folds its slabs -- stride n_params, up to 512 of them -- with k_mlp_reduce<1> / <2> (mlp_tail.hip): the same three
    replays over the wide workspace, at slab counts on both sides of the <1> / <2> threshold."""
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


def replay_reduce(slabs, halves=1):
    """k_mlp_reduce's tree in float32, per parameter, over (n_slabs, n_params) slabs: k_mlp_reduce_x4 and k_mlp_reduce<1> with
    halves = 1, k_mlp_reduce<2> (more than 256 slabs: 32 rows per group, two halves of 16) with halves = 2."""
    n_slabs, n = slabs.shape
    assert n_slabs <= 256 * halves
    zero = np.zeros(n, np.float32)
    t = np.zeros(n, np.float32)
    for grp in range(16):
        x = [slabs[grp + 16 * j] if grp + 16 * j < n_slabs else zero for j in range(16 * halves)]
        acc = None
        for h in range(halves):
            a4 = [((x[16 * h + k] + x[16 * h + k + 4]) + x[16 * h + k + 8]) + x[16 * h + k + 12] for k in range(4)]
            ah = (a4[0] + a4[1]) + (a4[2] + a4[3])
            acc = ah if h == 0 else acc + ah
        t = t + acc
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


def _setup(D, A, cont, B=262144, seed=0, hidden=64, layers=2):
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(D, (A,) if cont else A, hidden, layers, 0.0, cont).cuda()
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


# (D, Gaussian head, M, A); A = None: 6 actions for the Gaussian head, 4 logits for the Categorical one
CASES = [(D, cont, M, None) for D in (64, 17) for cont in (True, False) for M in (131072, 16384, 33, 1071, 8200)]
CASES.append((17, True, 1071, 3))       # n_params = 10887 = 3 (mod 4); the buckets above are 1 (mod 4)
CASE_IDS = [f"D{D}-{'cont' if c else 'disc'}-{f'A{A}-' if A else ''}M{M}" for D, c, M, A in CASES]


def _buffer_rows(M):
    """Rows of the rollout buffer a case draws its minibatch (and the slice after it) from: the small M need no 262144."""
    return 262144 if M > 8200 else 32768


def _check_tail_replays(H, ws, off, n_slabs, stride, halves, obs, act, rec, idx, bucket, lay, g, sc):
    """The three replays over workspace ws, whose slabs (n_slabs rows of `stride` floats at off["slabs"]) and loss partials
    mlp_ppo_step has just written for the slice idx: its gradient g and scalars sc against them; then a whole minibatch on a copy of
    the weights, and the clip's partial sums that its reduce leaves at off["sq_part"]."""
    n, M = lay["n_params"], idx.numel()
    slabs = ws[off["slabs"]:off["slabs"] + 4 * n_slabs * stride].view(torch.float32).view(n_slabs, stride)[:, :n].cpu().numpy()
    assert np.isfinite(slabs).all()
    want = replay_reduce(slabs, halves)
    got = g[:n].cpu().numpy()
    bad = np.flatnonzero(want.view(np.uint32) != got.view(np.uint32))
    print(f"  slabs {n_slabs} (halves {halves}), n_params {n} = {n % 4} (mod 4), {n % 64} (mod 64): mismatching gradient elements {bad.size}")
    assert bad.size == 0, (bad[:8], want[bad[:8]], got[bad[:8]])
    lp = ws[off["loss_part"]:off["loss_part"] + 8 * 8 * n_slabs].view(torch.float64).view(n_slabs, 8).cpu().numpy()
    want_sc = replay_scalars(lp, n_slabs, M, 0.01, 0.5)
    got_sc = sc.cpu().numpy()
    print(f"  loss scalars {got_sc.tolist()}, replay {want_sc.tolist()}")
    assert np.array_equal(want_sc.view(np.uint32), got_sc.view(np.uint32)), (want_sc, got_sc)
    # a whole minibatch on a copy of the weights: the same slabs (static tiles, the step reads the weights before the optimizer
    # launch), and the reduce now also leaves the clip's partial sums
    dev = torch.device("cuda")
    p2 = bucket.flat_param.clone()
    g2 = torch.empty_like(bucket.flat_grad)
    m_, v_ = torch.zeros_like(p2), torch.zeros_like(p2)
    sc2, norm = torch.empty(9, device=dev), torch.empty(1, device=dev)
    keep = side_shuffle(H)
    H.mlp_ppo_minibatch(obs, act, rec, idx, p2, lay, g2, 0.2, 0.01, 0.5, True, 1, sc2, m_, v_, torch.tensor([3e-4], device=dev),
                        torch.zeros(1, device=dev), 0.5, (0.9, 0.999), 1e-5, norm)
    torch.cuda.synchronize()
    del keep
    n_red = (n + 63) // 64
    got_sq = ws[off["sq_part"]:off["sq_part"] + 8 * n_red].view(torch.float64).cpu().numpy()
    want_sq = replay_sq_part(want)
    bad_sq = np.flatnonzero(want_sq.view(np.uint64) != got_sq.view(np.uint64))
    print(f"  clip partial sums differing from the replay {bad_sq.size} of {n_red}")
    assert bad_sq.size == 0, (bad_sq[:8], want_sq[bad_sq[:8]], got_sq[bad_sq[:8]])
    assert np.array_equal(want_sc.view(np.uint32), sc2.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("D,cont,M,A", CASES, ids=CASE_IDS)
def test_gradient_is_the_fixed_tree_over_the_slabs(D, cont, M, A, monkeypatch):
    monkeypatch.setenv("AURPPO_STATIC_TILES", "1")
    monkeypatch.setenv("AURPPO_K7_VARIANT", "3")
    A = A or (6 if cont else 4)
    H, pol, bucket, obs, act, rec = _setup(D, A, cont, _buffer_rows(M))
    lay = H.mlp_layout(pol, bucket)
    assert lay is not None and not lay.get("wide")
    n = lay["n_params"]
    idx = torch.randperm(obs.shape[0], device="cuda")[:M].int()
    keep = side_shuffle(H)
    g = torch.full_like(bucket.flat_grad, float("nan"))
    sc = H.mlp_ppo_step(obs, act, rec, idx, bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1)
    torch.cuda.synchronize()
    ws = H._ws_cache[("mlp", torch.cuda.current_device())]
    grid = k7_grid(M)
    print(f"D={D} cont={cont} A={A} M={M}: grid {grid}")
    _check_tail_replays(H, ws, ws_layout(n), grid, slab_stride(n), 1, obs, act, rec, idx, bucket, lay, g, sc)
    del keep


@pytest.mark.parametrize("D,cont,M,A", CASES, ids=CASE_IDS)
def test_chained_operand_copies_match_a_fresh_prepare(D, cont, M, A, monkeypatch):
    monkeypatch.setenv("AURPPO_K7_VARIANT", "3")
    A = A or (6 if cont else 4)
    H, pol, bucket, obs, act, rec = _setup(D, A, cont, _buffer_rows(M))
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


K_MAX_SLABS, K_OP_FLOATS, K_OP3_ELEMS = 2 * K_MAX_GRID, 2 * 3 * 2 * 16 * 64 * 16, 2 * 3 * 2 * 4 * 8 * 3 * 64 * 8     # mlp_wide.h, mlp_common.h


def wide_slab_cap(hidden, D):
    """mlp_wide.hip wide_slab_cap: slabs the workspace holds."""
    return K_MAX_SLABS if hidden <= 64 and D <= 64 else K_MAX_GRID // 2


def wide_ws_layout(n_params, hidden, D):
    """Byte offsets of mlp_wide.h's workspace carve-up (wide_ws), and the size aurppo_mlp_wide_workspace_bytes reports: the regions'
    sizes plus the slack of those that are no multiple of 64 bytes (mlp_common.h WsCarver)."""
    n_red = (n_params + 63) // 64
    sizes = [("stats", 8 * 2 * K_STAT_BLOCKS, 0), ("loss_part", 8 * 8 * K_MAX_SLABS, 0), ("wop", 4 * K_OP_FLOATS, 0), ("tile_counter", 4 * 16, 0),
             ("slabs", 4 * wide_slab_cap(hidden, D) * n_params, 64), ("sq_part", 8 * n_red, 128), ("wop3", 2 * K_OP3_ELEMS, 64)]
    off, at, total = {}, 0, 0
    for name, nbytes, slack in sizes:
        off[name] = at
        at += _r64(nbytes)
        total += nbytes + slack
    off["bytes"] = total
    return off


def k7w_pairs(M, hidden, D):
    """mlp_wide.hip wide_step_impl: how many slabs (both-net workgroups, or pairs of one-net workgroups) a launch at minibatch M writes."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    spare = int(os.environ.get("AURPPO_MLP_SPARE_CUS", "8") or 8)
    spare = spare if spare >= 0 else 8
    dual = hidden <= 64 and D <= 64
    pairs = 2 * (cus - spare) if dual else (cus - spare) // 2
    pairs = min(pairs, K_MAX_SLABS if dual else K_MAX_GRID // 2, (M + 31) // 32)
    return max(pairs, 1)


# (layers, hidden, D, A, Gaussian head, M): one layer of 64 -- both nets in a workgroup, n_params 2567 = 3 (mod 4), 7 (mod 64) -- at 2,
# 17, 257 (k_mlp_reduce<2>, one row in the second half) and 2 (CUs - spare) slabs; two layers of 128 -- a net per workgroup,
# k_mlp_reduce<1> -- at 17 and (CUs - spare) / 2
WIDE_B = 16384
WIDE_CASES = [(1, 64, 17, 3, True, M) for M in (33, 530, 8200, 16384)] + [(2, 128, 17, 4, False, M) for M in (530, 4000)]


@pytest.mark.parametrize("layers,hidden,D,A,cont,M", WIDE_CASES,
                         ids=[f"{nl}x{h}-D{D}-{'cont' if c else 'disc'}-M{M}" for nl, h, D, A, c, M in WIDE_CASES])
def test_wide_gradient_is_the_fixed_tree_over_the_slabs(layers, hidden, D, A, cont, M, monkeypatch):
    monkeypatch.setenv("AURPPO_STATIC_TILES", "1")
    H, pol, bucket, obs, act, rec = _setup(D, A, cont, WIDE_B, hidden=hidden, layers=layers)
    lay = H.mlp_layout(pol, bucket)
    assert lay is not None and lay.get("wide")
    n = lay["n_params"]
    off = wide_ws_layout(n, hidden, D)
    assert off["bytes"] == H._lib_or_raise().aurppo_mlp_wide_workspace_bytes(n, hidden, D)
    idx = torch.randperm(obs.shape[0], device="cuda")[:M].int()
    keep = side_shuffle(H)
    g = torch.full_like(bucket.flat_grad, float("nan"))
    sc = H.mlp_ppo_step(obs, act, rec, idx, bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1)
    torch.cuda.synchronize()
    ws = H._ws_cache[("mlp_wide", torch.cuda.current_device())]
    pairs = k7w_pairs(M, hidden, D)
    print(f"{layers} x {hidden}, D={D} cont={cont} A={A} M={M}: slabs {pairs}, kernel {H.k7w_kernel_name(hidden, D, layers)}")
    _check_tail_replays(H, ws, off, pairs, n, 1 if pairs <= K_MAX_GRID else 2, obs, act, rec, idx, bucket, lay, g, sc)
    del keep
