"""Do two builds of the library compute the same BITS in the fused MLP kernels (K7, K7w, K8, K8w, their reduce / optimizer launches),
the head kernels (K13, K14), the layered rollout step and the device CartPole (K15, K16)?
    AURPPO_LIB=<build> python tools/build_bitdiff.py run OUT.npz     (once per build, each in a process of its own)
    python tools/build_bitdiff.py cmp A.npz B.npz                    (raw bytes of every array; exit 1 + the first that differs)
`run` drives every build of the step (K7 ids 3, 2; K7w ids 1, 3, 2) with AURPPO_STATIC_TILES=1 (a fixed summation order; the
counter-dealt order is not reproducible by construction) over the smallest shapes that reach every path, at M = 1, 65, 1071 (17 slabs
for K7, 34 for the 64-wide K7w shapes: neither one, two nor the full grid) and 70001, and
stores gradient, scalars and the whole workspace after mlp_ppo_step; parameters, moments, norms, step count and workspace after two
chained mlp_ppo_minibatch calls (the first names next_idx) and after mlp_ppo_grad + mlp_ppo_apply (K7); the mlp_act outputs.  The
workspace is zero-filled before each sequence, so that bytes no kernel writes are equal across processes.
The head kernels run at every threads-per-row build (H = 32, 96, 256, 512, 1024: 8, 32, 64, 128, 256), Gaussian heads of 1 and 16
actions, Categorical heads of 2 and 16, M = N = 1, 65, 4099: head_ppo with records beside actions and packed (where the action row
fits a packed record) -- gz of both nets, gradient, scalars, workspace (K13's grid depends on (M, H) only, so its slabs repeat) --
head_act with noise and for the value alone, and mlp_layered_prepare + mlp_layered_act on layered policies of those widths.
The CartPole section builds the default Categorical 2 x 64 policy over D = 4, A = 2 (the actor's last layer scaled so that both actions
occur), resets a device CartPole under a fixed seed (every third env 5 steps short of truncation, every third entering as done) and runs
cartpole_rollout at (N, T) = (1, 1), (33, 5), (70, 40): the six buffer tensors (poisoned first), the episode table, next_obs, next_done
and the env's state, step counts and episode numbers behind K16; then one cartpole_step (K15) from there."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# (layers, hidden, D, A, Gaussian head, packed records)
K7_SHAPES = [(2, 64, 64, 6, True, False), (2, 64, 17, 3, True, False), (2, 64, 64, 12, True, True), (2, 64, 32, 5, False, False)]
# (2 x 100 over 17: k_mlpw3_step's run-time trip counts over a ragged state, and under variant 2 k_mlpw_step's own-out-block dW_1;
# 2 x 96 over 100: the <., 6, 8> build; 3 x 128 Categorical: the three-layer builds' other head)
K7W_SHAPES = [(1, 64, 64, 6, True, False), (3, 64, 64, 6, True, False), (3, 128, 64, 6, True, False), (2, 128, 128, 16, True, False),
              (1, 96, 64, 4, False, False), (2, 100, 17, 4, True, False), (2, 96, 100, 6, True, False), (3, 128, 64, 5, False, False)]
MS, B = (1, 65, 1071, 70001), 71000
HEAD_HS, HEAD_KINDS, HEAD_NS, HEAD_B = (32, 96, 256, 512, 1024), ((1, True), (16, True), (2, False), (16, False)), (1, 65, 4099), 4200
# (layers, hidden, D): widths no fused kernel takes, or (32, 96) a state no fused kernel takes
LAYERED_SHAPES = [(2, 32, 144), (1, 96, 144), (2, 256, 16), (1, 512, 16), (1, 1024, 16)]
# K16's (N, T): one env and one step; two tiles, the second ragged; three tiles over 40 steps (tests/test_cartpole_gpu.py's shapes)
CART_SHAPES, CART_SEED = [(1, 1), (33, 5), (70, 40)], 21


def head_layout(H, pol, bucket, Hd, A, cont):
    """The layout hip_ops.head_ppo / head_act take for a one-layer policy of any width (the head kernels take every H a multiple of
    32, whichever kernel owns the policy's update); tools/head_time.py uses it too."""
    seq, n = H._mlp_structure(pol, bucket)[:2]
    return dict(offsets=seq, n_params=n, D=pol.actor.net[0].weight.shape[1], A=A, continuous=cont, hidden=Hd, num_layers=1, layered=True)


def run(out_path):
    os.environ["AURPPO_TEST_KNOBS"] = "1"       # the library re-reads its knobs on every call: one process runs every build
    os.environ["AURPPO_STATIC_TILES"] = "1"
    import torch
    from aur_ppo_amd import _lib
    if os.environ.get("AURPPO_LIB"):
        _lib.LIB_PATH = os.environ["AURPPO_LIB"]
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    lib, dev, out = _lib.load(), torch.device("cuda:0"), {}

    def keep(key, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            out[key + name] = t.detach().cpu().contiguous().view(-1).numpy().view(np.uint8).copy()

    def policy(D, A, cont, Hd, NL):
        torch.manual_seed(1000 * NL + Hd + D + A)                       # CPU generator: the same inputs in every process
        pol = actor_critic(D, (A,) if cont else A, Hd, NL, 0.0, cont)
        with torch.no_grad():
            for p in pol.parameters():
                p.add_(0.05 * torch.randn_like(p))
        return pol, FlatBucket(pol.to(dev).parameters())

    def noise_for(N, A, cont):
        return (torch.randn(N, A) if cont else torch.rand(N)).to(dev)

    def case(tag, NL, Hd, D, A, cont, packed):
        pol, bucket = policy(D, A, cont, Hd, NL)
        lay = H.mlp_layout(pol, bucket)
        assert lay is not None and lay["wide"] == tag.startswith("k7w"), (tag, lay)
        n, nb, flat = lay["n_params"], bucket.flat_param.numel(), bucket.flat_param
        obs = torch.randn(B, D).to(dev)
        act = (torch.randn(B, A) if cont else torch.randint(0, A, (B,)).float()).to(dev)
        rec = torch.stack([-1.0 + 0.3 * torch.randn(B), 2 * torch.randn(B), torch.randn(B), torch.randn(B)], 1).contiguous().to(dev)
        perm, p0 = torch.randperm(B).int().to(dev), flat.clone()
        if packed:
            act, rec = None, H.pack_records(rec, act)
        ws_bytes = lib.aurppo_mlp_wide_workspace_bytes(n, Hd, D) if lay["wide"] else lib.aurppo_mlp_workspace_bytes(n)
        ws = H._workspace("mlp_wide" if lay["wide"] else "mlp", ws_bytes, dev)

        def fresh():
            flat.copy_(p0)
            ws.zero_()
            return (torch.zeros(nb, device=dev), torch.zeros(nb, device=dev), torch.zeros(nb, device=dev),
                    torch.full((1,), 3e-3, device=dev), torch.zeros(1, device=dev), torch.zeros(2, 9, device=dev), torch.zeros(2, device=dev))

        for M in MS:
            key, pairs = f"{tag}/M{M}/", ((perm[:M].contiguous(), perm[M:2 * M].contiguous()), (perm[M:2 * M].contiguous(), None))
            g, m, v, lr, t, sc, norms = fresh()
            H.mlp_ppo_step(obs, act, rec, pairs[0][0], flat, lay, g, 0.2, 0.01, 0.5, True, 1, sc[0])
            keep(key + "step/", grad=g, scalars=sc, ws=ws[:ws_bytes])
            g, m, v, lr, t, sc, norms = fresh()
            for k, (idx, nxt) in enumerate(pairs):
                H.mlp_ppo_minibatch(obs, act, rec, idx, flat, lay, g, 0.2, 0.01, 0.5, True, 1, sc[k], m, v, lr, t, 0.5, (0.9, 0.999), 1e-5,
                                    norms[k:k + 1], next_idx=nxt, chained=k > 0)
            keep(key + "minibatch/", params=flat, exp_avg=m, exp_avg_sq=v, norms=norms, step=t, scalars=sc, ws=ws[:ws_bytes])
            if not lay["wide"]:
                g, m, v, lr, t, sc, norms = fresh()
                for k, (idx, nxt) in enumerate(pairs):
                    H.mlp_ppo_grad(obs, act, rec, idx, flat, lay, g, 0.2, 0.01, 0.5, True, 1, sc[k], t, chained=k > 0)
                    H.mlp_ppo_apply(flat, g, m, v, lay, lr, t, 0.5, (0.9, 0.999), 1e-5, norms[k:k + 1], rec=rec, next_idx=nxt)
                keep(key + "grad_apply/", params=flat, exp_avg=m, exp_avg_sq=v, norms=norms, step=t, scalars=sc, ws=ws[:ws_bytes])
            fresh()
            a_, lp_, v_ = H.mlp_act(obs[:M].contiguous(), (torch.randn(M, A) if cont else torch.rand(M)).to(dev), flat, lay)
            keep(key + "act/", actions=a_, logp=lp_, value=v_)

    def head_case(Hd, A, cont):
        pol, bucket = policy(16, A, cont, Hd, 1)
        lay = head_layout(H, pol, bucket, Hd, A, cont)
        act = (torch.randn(HEAD_B, A) if cont else torch.randint(0, A, (HEAD_B,)).float()).to(dev)
        rec = torch.stack([-1.0 + 0.3 * torch.randn(HEAD_B), 2 * torch.randn(HEAD_B), torch.randn(HEAD_B), torch.randn(HEAD_B)], 1).contiguous().to(dev)
        perm = torch.randperm(HEAD_B).int().to(dev)
        forms = [("", act, rec)] + ([("packed/", None, H.pack_records(rec, act))] if (A if cont else 1) <= 12 else [])
        for M in HEAD_NS:
            key = f"head/H{Hd}-A{A}{'' if cont else 'c'}/M{M}/"
            hA, hC = torch.tanh(torch.randn(M, Hd)).to(dev), torch.tanh(torch.randn(M, Hd)).to(dev)
            nz = noise_for(M, A, cont)
            ws_bytes = lib.aurppo_head_ppo_workspace_bytes(M, Hd, A)
            ws = H._workspace("head", ws_bytes, dev)
            for form, a_, r_ in forms:
                ws.zero_()
                g, gzA, gzC = torch.zeros_like(bucket.flat_grad), torch.zeros_like(hA), torch.zeros_like(hC)
                sc = H.head_ppo(hA, hC, a_, r_, perm[:M].contiguous(), bucket.flat_param, lay, g, 0.2, 0.01, 0.5, True, 1, gzA=gzA, gzC=gzC)
                keep(key + "ppo/" + form, gzA=gzA, gzC=gzC, grad=g, scalars=sc, ws=ws[:ws_bytes])
            a_, lp_, v_ = H.head_act(hA, hC, nz, bucket.flat_param, lay)
            keep(key + "act/", actions=a_, logp=lp_, value=v_)
            keep(key + "act/value_only/", value=H.head_act(None, hC, None, bucket.flat_param, lay)[2])

    def layered_case(NL, Hd, D, A, cont):
        pol, bucket = policy(D, A, cont, Hd, NL)
        lay = H.mlp_layered_layout(pol, bucket)
        assert lay is not None, (NL, Hd, D)
        wop = H.mlp_layered_prepare(bucket.flat_param, lay)
        for N in HEAD_NS:
            key = f"layered/{NL}x{Hd}-D{D}-A{A}{'' if cont else 'c'}/N{N}/"
            obs = torch.randn(N, D).to(dev)
            a_, lp_, v_ = H.mlp_layered_act(obs, noise_for(N, A, cont), bucket.flat_param, lay, wop=wop)
            keep(key + "act/", actions=a_, logp=lp_, value=v_)
            keep(key + "act/value_only/", value=H.mlp_layered_act(obs, None, bucket.flat_param, lay, wop=wop)[2])

    def cartpole_case(N, T):
        from aur_ppo_amd.envs import CartPoleDeviceVecEnv
        pol, bucket = policy(4, 2, False, 64, 2)
        with torch.no_grad():
            pol.actor.net[4].weight.mul_(40.0)          # logits that move with the state, so both actions occur
        lay = H.mlp_layout(pol, bucket)
        assert H.cartpole_rollout_ok(lay), lay
        env = CartPoleDeviceVecEnv(N, dev, seed=CART_SEED)
        state0, _, _ = env.get_state()
        obs = env.set_state(state0, np.where(np.arange(N) % 3 == 1, 495, 0)).contiguous()    # every third env truncates inside T >= 5
        done = (torch.arange(N) % 3 == 0).float().to(dev)
        noise = torch.rand(T, N).to(dev)
        z = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device=dev)
        buf = dict(states=z(T, N, 4), terminals=z(T, N), actions=z(T, N), log_probs=z(T, N), values=z(T, N), rewards=z(T, N))
        table = env.begin_rollout(T)
        H.cartpole_rollout(env.native_state(), bucket.flat_param, lay, noise, buf["states"], buf["terminals"], buf["actions"], buf["log_probs"],
                           buf["values"], buf["rewards"], table, obs, done)
        key = f"cartpole/N{N}-T{T}/"
        keep(key + "rollout/", ep_len=table, next_obs=obs, next_done=done, env_state=env.state, env_steps=env.steps, env_episode=env.episode, **buf)
        row = env.begin_rollout(1)                              # K15 alone, from where K16 left the envs
        o2, r2, d2, _, _ = env.step(buf["actions"][T - 1])
        keep(key + "step/", obs=o2, reward=r2, done=d2, ep_len=row, env_state=env.state, env_steps=env.steps, env_episode=env.episode)

    for N, T in CART_SHAPES:
        cartpole_case(N, T)
    for Hd in HEAD_HS:
        for A, cont in HEAD_KINDS:
            head_case(Hd, A, cont)
    for k, (NL, Hd, D) in enumerate(LAYERED_SHAPES):
        layered_case(NL, Hd, D, *HEAD_KINDS[k % len(HEAD_KINDS)])
    for knob, shapes in (("AURPPO_K7_VARIANT", K7_SHAPES), ("AURPPO_K7W_VARIANT", K7W_SHAPES)):
        for s in shapes:
            dual = knob == "AURPPO_K7W_VARIANT" and lib.aurppo_k7w_kernel(s[1], s[2]) == 1     # K7w id 1: the knob does not matter
            for variant in ("1",) if dual else ("3", "2"):
                os.environ[knob] = variant
                case(f"{'k7w' if 'K7W' in knob else 'k7'}-{variant}/{s[0]}x{s[1]}-D{s[2]}-A{s[3]}{'' if s[4] else 'c'}", *s)
    np.savez(out_path, **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values()) / 1e6:.0f} MB -> {out_path}")


def cmp(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        print("the two runs hold different arrays:", sorted(set(a.files) ^ set(b.files))[:5])
        return 1
    for k in a.files:
        if not np.array_equal(a[k], b[k]):
            bad = np.flatnonzero(a[k] != b[k]) if a[k].shape == b[k].shape else []
            print(f"DIFFERENT: {k}: {len(bad)} of {a[k].size} bytes, the first at byte {bad[0] if len(bad) else '-'}")
            return 1
    print(f"identical: {len(a.files)} arrays")
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else cmp(sys.argv[2], sys.argv[3]))
