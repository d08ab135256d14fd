// K7 host side + the small kernels around the fused PPO minibatch step for the reference's MLP actor-critic
// (src/models/actor_critic.py:8-51 over src/nets/nets.py:19-53: two Tanh hidden layers of 64, Gaussian head with a
// state-independent log-std or Categorical head): gather (a7) + policy/value forward (a8) + advantage normalisation and
// clipped-surrogate loss (a9/a10) + back-propagation, producing the flat parameter-gradient bucket and the 9 loss scalars.
//
// Why: rocprof of the per-op path (profiles/r01) shows ~100 small kernels per minibatch moving ~2 GB through HBM for
// 11 GFLOP of work.  A minibatch reads each sample's observation row and its packed record ONCE (through the
// permutation, so K3's copy disappears too) and writes only per-workgroup gradient slabs; every activation lives in
// LDS / registers.  The step kernels themselves: mlp2.hip (k_mlp_step2, fp32 MFMA) and mlp3.hip (k_mlp_step3, the same
// step on bf16 MFMAs over three-way bf16 splits of every fp32 operand).  Here:
//   * k_adv_stats_idx  -- advantage partial sums of a minibatch + operand-order copies of the weights the step streams;
//   * k_mlp_act (K8)   -- the rollout step (forward only);
//   * k_pack_rec64     -- record + action row in one 64-B line per sample;
//   * the workspace carve-up (ws_view), the step and apply host paths and K7's C entries.
// What runs behind the step kernel -- the slab reduce, then clip + Adam with the operand copies' refresh and the next minibatch's
// statistics -- is mlp_tail.hip, shared with K7w (mlp_wide.hip).
// (Round 1-2's one-tile-set kernel k_mlp_step -- 4 waves, 221 us -- was kept for A/B until round 3 and is gone.)
#include <stdlib.h>

#include "bf16x3.h"
#include "mlp_act.h"
#include "mlp_tail.h"

using namespace aurppo_mlp;

namespace {

// Also lays out W1 of both nets in the B-operand order of k_mlp_step2's layer-1 MFMA chain (w1op != nullptr, variant 2; the layout:
// mlp_common.h, w1op_index).  The workgroups past the first n_stat build k_mlp_step3's bf16-plane copies of W1 / W2 instead (variant
// 3; this was a launch of its own).
__global__ __launch_bounds__(256) void k_adv_stats_idx(const float4* __restrict__ rec, int rec_stride,
                                                       const int32_t* __restrict__ idx,
                                                       int M, double (*__restrict__ stats)[2], const float* __restrict__ params,
                                                       MlpLayout L, int D, float* __restrict__ w1op,
                                                       unsigned short* __restrict__ wop3, int n_stat,
                                                       unsigned* __restrict__ tile_counter) {
    if ((int)blockIdx.x >= n_stat) {
        bf3::wop3_prepare(params, L.w1, L.w2, D, wop3, (blockIdx.x - n_stat) * kThreads + threadIdx.x, (gridDim.x - n_stat) * kThreads);
        return;
    }
    __shared__ double sc[2][kThreads / kWave];
    if (blockIdx.x == 0 && threadIdx.x < 2) tile_counter[threadIdx.x] = 0u;
    if (w1op) {
        for (int e = blockIdx.x * kThreads + threadIdx.x; e < kW1opFloats; e += n_stat * kThreads) {
            const W1opPlace q = w1op_place(e);
            w1op[e] = q.col < D ? params[L.w1[q.net] + q.row * D + q.col] : 0.0f;
        }
    }
    double s = 0.0, q = 0.0;
    adv_partial_sums(rec, rec_stride, idx, M, blockIdx.x * kThreads + threadIdx.x, n_stat * kThreads, s, q);
    const double bs = block_sum<kThreads / kWave>(s, sc[0]);
    const double bq = block_sum<kThreads / kWave>(q, sc[1]);
    if (threadIdx.x == 0) {
        stats[blockIdx.x][0] = bs;
        stats[blockIdx.x][1] = bq;
    }
}

// ---- K8: forward-only sibling of K7 for the rollout step (src/ppo.py:103-108: policy.evaluate(next_obs) under
// no_grad, then buffer.values / actions / log_probs [step] = ...).  One workgroup per 32-row tile: both nets'
// forward pass as in K7, then 32 lanes sample the action from caller-supplied noise (a ~ mu + sigma*eps for the
// Gaussian head, inverse CDF of softmax(logits) at u for the Categorical head), form its log-prob and write
// action / log-prob / value straight into the rollout buffer rows.  With noise == nullptr only the value is
// produced (the bootstrap policy.value(next_obs), src/ppo.py:161).
struct ActArgs {
    const float* obs;     // (N, D)
    const float* noise;   // (N, A) standard normal | (N,) uniform [0,1) | nullptr
    const float* params;
    float* actions;       // (N, A) | (N,)
    float* logp;          // (N,)
    float* value;         // (N,)
    int N, D, A, continuous;
    MlpLayout L;
};

// K8 takes its LDS plan from mlp_act.h -- every pointer below is ActLds's offset of that member, the launch's byte count is
// ActLds::bytes(true), so a member cannot be added to one and not the other -- but keeps its own text of the weight staging and the
// three layers.  On act_stage_weights / act_forward it computed the same bits (tools/build_bitdiff.py: 2250 arrays identical) and
// ran slower than the parent build in every one of five alternating rounds: 8.67-8.71 us for 8.61-8.65 us (Gaussian head), 9.90-9.92 us
// for 9.83-9.85 us (Categorical), N = 4096, tools/head_time.py; profiles/refactor_act_forward.txt, section 4.  So a change to the
// staging or the layers below is a change to mlp_act.h too: tests/test_cartpole_gpu.py (K16 == T x (K8, K15), no tolerance) is what
// holds the two texts together.
__global__ __launch_bounds__(256, 1) void k_mlp_act(const ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sX = lds + ActLds::at(ActLds::kX);
    float* sH1 = lds + ActLds::at(ActLds::kH1);
    float* sH2 = lds + ActLds::at(ActLds::kH2);
    float* sW1 = lds + ActLds::at(ActLds::kW1);
    float* sW2 = lds + ActLds::at(ActLds::kW2);
    float* sW3 = lds + ActLds::at(ActLds::kW3);
    float* sOut = lds + ActLds::at(ActLds::kOut);
    float* sB1 = lds + ActLds::at(ActLds::kB1);
    float* sB2 = lds + ActLds::at(ActLds::kB2);
    float* sB3 = lds + ActLds::at(ActLds::kB3);
    float* sLs = lds + ActLds::at(ActLds::kLs);
    float* sSd = lds + ActLds::at(ActLds::kSd);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int net = wave >> 1, cb = wave & 1;
    const int D = a.D, A = a.A;
    const int out_dim[2] = {A, 1};
    const int row0 = blockIdx.x * R;
    // Staging: every element's address comes from shifts of a flat index over rows padded to 64 columns (no division,
    // no zero-fill pass), and all of a thread's loads are independent, so they go out together -- the kernel is a
    // latency chain (launch, staging, three layers, sampling) and this was its longest link.
#pragma unroll
    for (int u = 0; u < R * H / kThreads; ++u) {
        const int e = tid + u * kThreads, r = e >> 6, c = e & 63;
        // branch-free: a padding lane reads a clamped (valid) element and masks it -- a load under a divergent
        // condition makes the compiler wait for everything in flight
        const int rr = row0 + r < a.N ? row0 + r : a.N - 1, cc = c < D ? c : D - 1;
        const float x = a.obs[(size_t)rr * D + cc];
        sX[r * LD + c] = (c < D && row0 + r < a.N) ? x : 0.0f;
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int u = 0; u < H * H / kThreads; ++u) {
            const int e = tid + u * kThreads, o = e >> 6, c = e & 63;
            const float w1v = a.params[a.L.w1[n] + o * D + (c < D ? c : D - 1)];
            const float w2v = a.params[a.L.w2[n] + e];
            sW1[(n * H + o) * LD + c] = c < D ? w1v : 0.0f;
            sW2[(n * H + o) * LD + c] = w2v;
        }
#pragma unroll
        for (int u = 0; u < AP * H / kThreads; ++u) {
            const int e = tid + u * kThreads, o = e >> 6, i = e & 63;
            sW3[(n * AP + o) * LD + i] = o < out_dim[n] ? a.params[a.L.w3[n] + o * H + i] : 0.0f;
        }
        if (tid < H) {
            sB1[n * H + tid] = a.params[a.L.b1[n] + tid];
            sB2[n * H + tid] = a.params[a.L.b2[n] + tid];
        }
        if (tid < AP) sB3[n * AP + tid] = tid < out_dim[n] ? a.params[a.L.b3[n] + tid] : 0.0f;
    }
    if (tid < AP) {
        const float ls = (a.continuous && tid < A) ? a.params[a.L.logstd + tid] : 0.0f;
        sLs[tid] = ls;
        sSd[tid] = expf(ls);
    }
    __syncthreads();
    {
        f32x16 acc = zero16();
        const float* W = sW1 + (net * H + cb * 32) * LD;
        mma32<H>(acc, [&](int i, int k) { return sX[i * LD + k]; }, [&](int k, int j) { return W[j * LD + k]; });
        const int col = cb * 32 + (lane & 31);
        const float bias = sB1[net * H + col];
#pragma unroll
        for (int e = 0; e < 16; ++e) sH1[(net * R + acc_row(e, lane)) * LD + col] = tanh_fast(acc[e] + bias);
    }
    __syncthreads();
    {
        f32x16 acc = zero16();
        const float* W = sW2 + (net * H + cb * 32) * LD;
        const float* Hin = sH1 + net * R * LD;
        mma32<H>(acc, [&](int i, int k) { return Hin[i * LD + k]; }, [&](int k, int j) { return W[j * LD + k]; });
        const int col = cb * 32 + (lane & 31);
        const float bias = sB2[net * H + col];
#pragma unroll
        for (int e = 0; e < 16; ++e) sH2[(net * R + acc_row(e, lane)) * LD + col] = tanh_fast(acc[e] + bias);
    }
    __syncthreads();
    {
        const float* W = sW3 + net * AP * LD;
        const float* Hin = sH2 + (net * R + cb * 16) * LD;
        const f32x4 acc = mma16<H>([&](int i, int k) { return Hin[i * LD + k]; },
                                   [&](int k, int j) { return W[j * LD + k]; });
        const int col = lane & 15;
        const float bias = sB3[net * AP + col];
#pragma unroll
        for (int e = 0; e < 4; ++e) sOut[(net * R + cb * 16 + 4 * (lane >> 4) + e) * LDO + col] = acc[e] + bias;
    }
    __syncthreads();
    if (a.noise && a.continuous) {
        // 8 lanes per row, action dims lj and lj + 8 per lane; the log-prob terms are formed as evaluate() forms them
        // and folded with DPP moves
        const int r = tid >> 3, lj = tid & 7, n = row0 + r;
        const bool live = n < a.N;
        const float* mu = sOut + r * LDO;
        float lp = 0.0f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = lj + 8 * q;
            if (live && k < A) lp += gauss_sample(mu[k], sSd[k], sLs[k], a.noise[(size_t)n * A + k], a.actions[(size_t)n * A + k]);
        }
        lp = sum8(lp);
        if (live && lj == 0) {
            a.logp[n] = lp;
            a.value[n] = sOut[(R + r) * LDO];
        }
        return;
    }
    if (tid < R && row0 + tid < a.N) {
        const int n = row0 + tid;
        const float* mu = sOut + tid * LDO;
        a.value[n] = sOut[(R + tid) * LDO];
        if (a.noise) {      // Categorical: the Gaussian head has returned above
            const float lse = cat_lse(mu, A);
            float lp;
            a.actions[n] = (float)cat_sample(mu, A, lse, a.noise[n], lp);
            a.logp[n] = lp;
        }
    }
}

}  // namespace

namespace {
struct WsView {   // carve-up of the caller's workspace
    double* stats;               // (kStatBlocks, 2) advantage partial sums of the prepared minibatch
    double* loss_part;           // (kMaxGrid, 8)
    float* slabs;                // (kMaxGrid, slab_stride(n_params)), 16-byte aligned
    unsigned long long* stamps;  // diagnostic build: (kMaxGrid, 44)
    float* w1op;                 // W1 in B-operand order
    unsigned* tile_counter;      // 16 words: the counters; words 8..11 carry Adam's bias corrections from the reduce to the optimizer launch
    double* sq_part;             // clip partial sums, one per k_mlp_reduce_x4 workgroup
    unsigned short* wop3;        // k_mlp_step3: bf16 planes of W1 / W2 in operand order
    size_t bytes;                // aurppo_mlp_workspace_bytes
};
WsView ws_view(void* workspace, int n_params) {
    WsCarver c(workspace);
    WsView v;
    v.stats = c.take<double>(sizeof(double) * 2 * kStatBlocks);
    v.loss_part = c.take<double>(sizeof(double) * 8 * kMaxGrid);
    v.slabs = c.take<float>(sizeof(float) * (size_t)kMaxGrid * (size_t)slab_stride(n_params), 64);
    v.stamps = c.take<unsigned long long>(sizeof(unsigned long long) * 44 * kMaxGrid);
    v.w1op = c.take<float>(sizeof(float) * kW1opFloats);
    v.tile_counter = c.take<unsigned>(sizeof(unsigned) * 16);
    v.sq_part = c.take<double>((sizeof(double) * (size_t)((n_params + 63) / 64) + 63) / 64 * 64, 64);
    v.wop3 = c.take<unsigned short>(mlp_step3_wop_bytes(), 64);
    v.bytes = c.bytes;
    return v;
}
}  // namespace

extern "C" size_t aurppo_mlp_workspace_bytes(int n_params) { return ws_view(nullptr, n_params).bytes; }

static int mlp_step_impl(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                         int A, int continuous, int hidden, const float* params, const int* layout_h, int n_params, float* grads,
                         double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars,
                         void* workspace, void* stream, void* ev_begin, void* ev_end, const MlpTail* chain = nullptr) {
    if (const int rc = check_step_args("aurppo_mlp_ppo_step_f32", obs && rec && idx && params && layout_h && grads && out_scalars && workspace,
                                       actions, continuous, A, M, n_params, vloss_mode, [&]() -> int {
        AURPPO_REQUIRE(hidden == H, AURPPO_ESHAPE, "aurppo_mlp_ppo_step_f32: hidden_dim=%d (only %d is built)", hidden, H);
        AURPPO_REQUIRE(D >= 1 && D <= H, AURPPO_ESHAPE, "aurppo_mlp_ppo_step_f32: state_dim=%d must be 1..%d", D, H);
        AURPPO_REQUIRE(A >= 1 && A <= AP && (continuous || A >= 2), AURPPO_ESHAPE,
                       "aurppo_mlp_ppo_step_f32: action_dim=%d must be 1..%d (>= 2 logits for a Categorical head)", A, AP);
        return AURPPO_OK;
    }))
        return rc;
    AURPPO_REQUIRE(aligned_to(workspace, 16) && aligned_to(rec, 16), AURPPO_EINVAL,
                   "aurppo_mlp_ppo_step_f32: workspace / rec not 16-byte aligned");
    MlpArgs a;
    a.obs = obs; a.actions = actions; a.rec = reinterpret_cast<const float4*>(rec); a.idx = idx; a.params = params;
    a.rec_stride = actions ? 1 : 4;
    a.D = D; a.A = A;
    a.continuous = continuous ? 1 : 0;
    if (const int rc = fill_layout(a.L, layout_h, continuous, n_params, "aurppo_mlp_ppo_step_f32")) return rc;
    a.h = make_hyper(M, clip, ent_coef, vf_coef, norm_adv, vloss_mode);
    const WsView wv = ws_view(workspace, n_params);
    double* stats = wv.stats;
    a.stats = wv.stats;
    a.loss_part = wv.loss_part;
    a.slabs = wv.slabs;
    a.stamps = wv.stamps;
    hipStream_t s = (hipStream_t)stream;
    const int sb = stat_blocks_for(M);
    a.n_stat_blocks = sb;
    const AurppoKnobs& knobs = aurppo_knobs();
    // 2: k_mlp_step2 (f32 MFMA); 3: k_mlp_step3 (3 x bf16-split MFMA); normalised in api.hip::parse_knobs
    const int variant = knobs.k7_variant;
    a.w1op = wv.w1op;
    a.tile_counter = wv.tile_counter;
    a.static_tiles = knobs.static_tiles ? 1 : 0;
    a.wop3 = wv.wop3;
    if (!(chain && chain->chained)) {   // otherwise the previous chained call has prepared all of this
        // each variant's operand copies: W1 for k_mlp_step2 in the statistics workgroups, the bf16 planes for k_mlp_step3 in
        // 24 more (4 elements per thread)
        hipLaunchKernelGGL(k_adv_stats_idx, dim3(sb + (variant == 3 ? 24 : 0)), dim3(kThreads), 0, s, a.rec, a.rec_stride, idx, M,
                           reinterpret_cast<double (*)[2]>(stats), params, a.L, D, variant == 2 ? a.w1op : nullptr, wv.wop3, sb,
                           a.tile_counter);
        AURPPO_LAUNCH_CHECK("k_adv_stats_idx");
    }
    const int n_tiles = (M + R - 1) / R;
    // One persistent workgroup per CU, minus one CU per XCD (AURPPO_MLP_SPARE_CUS, default 8; workgroups are dealt
    // round-robin over the 8 XCDs): the single-workgroup shuffle kernels of the side stream then have a CU of
    // their own.  The kernel hands tiles out dynamically, but it fills a CU's register file, so a workgroup whose CU
    // is taken starts late; 8 spare CUs measured 3.86-3.93 ms per update against 4.09-4.10 ms with none.
    const int cus = aurppo_cu_count(kMaxGrid);
    if (cus < 0) return cus;
    int grid = cus - spare_cus();
    if (grid > kMaxGrid) grid = kMaxGrid;
    if (grid < 1) grid = 1;
    // A minibatch that every CU could take in ONE round of tiles (two per workgroup) but the spare-CU grid could not -- BASELINE
    // config 4's shard, 512 envs x 128 steps / 4 = 512 tiles against 2 x 248 -- gets all the CUs: the stragglers' second round
    // was a quarter of that launch (stamps at M = 16 384: tile loop 12.0 us median, 22.2 us for the sets that drew a second tile)
    if (n_tiles > 2 * grid && n_tiles <= 2 * cus && cus <= kMaxGrid) grid = cus;
    if (grid > (n_tiles + 1) / 2) grid = (n_tiles + 1) / 2;     // two tile sets per workgroup
    if (ev_begin) AURPPO_HIP_TRY(hipEventRecord((hipEvent_t)ev_begin, s));
    {
        const int rc = variant == 3 ? launch_mlp_step3(a, grid, s) : launch_mlp_step2(a, grid, s);
        if (rc != AURPPO_OK) return rc;
    }
    if (ev_end) AURPPO_HIP_TRY(hipEventRecord((hipEvent_t)ev_end, s));
    TailWork w = {};
    w.slabs = a.slabs; w.slab_strided = true; w.loss_part = a.loss_part; w.n_slabs = grid; w.n_params = n_params; w.h = a.h;
    w.grads = grads; w.out_scalars = out_scalars; w.sq_part = wv.sq_part; w.counters = a.tile_counter;
    w.rec = a.rec; w.rec_stride = a.rec_stride; w.stats = stats;
    // w1op is k_mlp_step2's operand; k_mlp_step3 never reads it, and the next non-chained call rebuilds it (k_adv_stats_idx)
    w.copies = operand_copies(n_params, &a.L, D, variant == 2 ? a.w1op : nullptr, variant == 3 ? wv.wop3 : nullptr);
    return launch_mlp_tail(w, chain, s);
}

extern "C" int aurppo_mlp_ppo_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx,
                                       int M, int D, int A, int continuous, int hidden, const float* params, const int* layout_h,
                                       int n_params, float* grads, double clip, double ent_coef, double vf_coef,
                                       int norm_adv, int vloss_mode, float* out_scalars, void* workspace, void* stream) {
    return mlp_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, params, layout_h, n_params, grads, clip, ent_coef,
                         vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, nullptr, nullptr);
}

extern "C" int aurppo_mlp_ppo_step_ev_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx,
                                          int M, int D, int A, int continuous, int hidden, const float* params, const int* layout_h,
                                          int n_params, float* grads, double clip, double ent_coef, double vf_coef,
                                          int norm_adv, int vloss_mode, float* out_scalars, void* workspace,
                                          void* stream, void* ev_begin, void* ev_end) {
    return mlp_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, params, layout_h, n_params, grads, clip, ent_coef,
                         vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, ev_begin, ev_end);
}

extern "C" int aurppo_mlp_ppo_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M,
                                            int D, int A, int continuous, int hidden, float* params, const int* layout_h,
                                            int n_params, float* grads, double clip, double ent_coef, double vf_coef,
                                            int norm_adv, int vloss_mode, float* out_scalars, float* exp_avg,
                                            float* exp_avg_sq, double max_norm, const float* lr_dev, float* step_dev,
                                            double beta1, double beta2, double eps, float* out_norm, const int32_t* next_idx,
                                            int next_M, int chained, void* workspace, void* stream) {
    AURPPO_REQUIRE(exp_avg && exp_avg_sq && lr_dev && step_dev && out_norm, AURPPO_EINVAL,
                   "aurppo_mlp_ppo_minibatch_f32: null optimizer pointer");
    AURPPO_REQUIRE(!next_idx || next_M > 0, AURPPO_ESHAPE, "aurppo_mlp_ppo_minibatch_f32: next_M=%d", next_M);
    MlpTail c;
    c.params_rw = params; c.exp_avg = exp_avg; c.exp_avg_sq = exp_avg_sq; c.max_norm = max_norm; c.lr_dev = lr_dev;
    c.step_dev = step_dev; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.out_norm = out_norm;
    c.next_idx = next_idx; c.next_M = next_idx ? next_M : 0; c.chained = chained ? 1 : 0; c.grad_only = 0;
    return mlp_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, params, layout_h, n_params, grads, clip, ent_coef,
                         vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, nullptr, nullptr, &c);
}

extern "C" int aurppo_mlp_ppo_grad_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                                       int A, int continuous, int hidden, const float* params, const int* layout_h, int n_params,
                                       float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                                       float* out_scalars, float* step_dev, int chained, void* workspace, void* stream) {
    AURPPO_REQUIRE(step_dev, AURPPO_EINVAL, "aurppo_mlp_ppo_grad_f32: null step_dev");
    MlpTail c = {};
    c.step_dev = step_dev; c.chained = chained ? 1 : 0; c.grad_only = 1;
    return mlp_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, params, layout_h, n_params, grads, clip, ent_coef,
                         vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, nullptr, nullptr, &c);
}

static int mlp_apply_impl(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* layout_h, int n_params, int D,
                          double grad_scale, const double* sq_part, int n_part, double max_norm, const float* lr_dev,
                          const float* step_dev, double beta1, double beta2, double eps, float* out_norm, const float* rec,
                          int rec_floats, const int32_t* next_idx, int next_M, void* workspace, void* stream) {
    AURPPO_REQUIRE(params && grads && exp_avg && exp_avg_sq && layout_h && lr_dev && step_dev && out_norm && workspace,
                   AURPPO_EINVAL, "aurppo_mlp_ppo_apply_f32: null pointer");
    AURPPO_REQUIRE(n_params > 0 && D >= 1 && D <= H, AURPPO_ESHAPE, "aurppo_mlp_ppo_apply_f32: n_params=%d D=%d",
                   n_params, D);
    AURPPO_REQUIRE(!next_idx || (next_M > 0 && rec && (rec_floats == 4 || rec_floats == 16)), AURPPO_ESHAPE,
                   "aurppo_mlp_ppo_apply_f32: next_M=%d rec_floats=%d", next_M, rec_floats);
    AURPPO_REQUIRE(aligned_to(workspace, 16) && (!rec || aligned_to(rec, 16)), AURPPO_EINVAL,
                   "aurppo_mlp_ppo_apply_f32: workspace / rec not 16-byte aligned");
    MlpLayout L;      // (the optimizer touches no log-std offset: the twelve weight / bias offsets are what is read and checked)
    if (const int rc = fill_layout(L, layout_h, 0, n_params, "aurppo_mlp_ppo_apply_f32")) return rc;
    const WsView wv = ws_view(workspace, n_params);
    AdamLaunch a = {};
    a.params = params; a.grads = grads; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.n_params = n_params;
    a.sq_part = sq_part; a.n_part = sq_part ? n_part : 0; a.gscale = (float)grad_scale;
    a.max_norm = max_norm; a.lr_dev = lr_dev; a.step_dev = step_dev; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.out_norm = out_norm;
    // (w1op is refreshed whichever variant runs: the next call may be made under the other one)
    a.copies = operand_copies(n_params, &L, D, wv.w1op, aurppo_knobs().k7_variant == 3 ? wv.wop3 : nullptr);
    a.rec = reinterpret_cast<const float4*>(rec); a.rec_stride = rec_floats == 16 ? 4 : 1;
    a.next_idx = next_idx; a.next_M = next_idx ? next_M : 0; a.stats = wv.stats;
    return launch_adam_chain(a, (hipStream_t)stream);
}

extern "C" int aurppo_mlp_ppo_apply_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* layout_h,
                                        int n_params, int D, double grad_scale, double max_norm, const float* lr_dev,
                                        const float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                        const float* rec, int rec_floats, const int32_t* next_idx, int next_M,
                                        void* workspace, void* stream) {
    return mlp_apply_impl(params, grads, exp_avg, exp_avg_sq, layout_h, n_params, D, grad_scale, nullptr, 0, max_norm, lr_dev, step_dev,
                          beta1, beta2, eps, out_norm, rec, rec_floats, next_idx, next_M, workspace, stream);
}

extern "C" int aurppo_mlp_ppo_apply_parts_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* layout_h,
                                              int n_params, int D, const double* sq_part, int n_part, double max_norm,
                                              const float* lr_dev, const float* step_dev, double beta1, double beta2, double eps,
                                              float* out_norm, const float* rec, int rec_floats, const int32_t* next_idx,
                                              int next_M, void* workspace, void* stream) {
    AURPPO_REQUIRE(sq_part && n_part > 0, AURPPO_EINVAL, "aurppo_mlp_ppo_apply_parts_f32: no partial sums");
    return mlp_apply_impl(params, grads, exp_avg, exp_avg_sq, layout_h, n_params, D, 1.0, sq_part, n_part, max_norm, lr_dev, step_dev,
                          beta1, beta2, eps, out_norm, rec, rec_floats, next_idx, next_M, workspace, stream);
}

namespace {
// rec64[b] = {rec4[b], actions[b][0 .. AW), 0 ...}: one 64-B line per sample for K7's record + action fetch
__global__ __launch_bounds__(256) void k_pack_rec64(const float4* __restrict__ rec4, const float* __restrict__ actions, int B,
                                                    int AW, float4* __restrict__ rec64) {
    const int i = blockIdx.x * 64 + (threadIdx.x >> 2), q = threadIdx.x & 3;   // 4 lanes per sample, one float4 each
    if (i >= B) return;
    float4 v;
    if (q == 0) {
        v = rec4[i];
    } else {
        const int k0 = 4 * (q - 1);
        const float* ar = actions + (size_t)i * AW;
        v.x = k0 + 0 < AW ? ar[k0 + 0] : 0.0f;
        v.y = k0 + 1 < AW ? ar[k0 + 1] : 0.0f;
        v.z = k0 + 2 < AW ? ar[k0 + 2] : 0.0f;
        v.w = k0 + 3 < AW ? ar[k0 + 3] : 0.0f;
    }
    rec64[(size_t)i * 4 + q] = v;
}
}  // namespace

extern "C" int aurppo_pack_records_f32(const float* rec4, const float* actions, int B, int action_floats, float* rec64,
                                       void* stream) {
    AURPPO_REQUIRE(rec4 && actions && rec64, AURPPO_EINVAL, "aurppo_pack_records_f32: null pointer");
    AURPPO_REQUIRE(B > 0 && action_floats >= 1 && action_floats <= 12, AURPPO_ESHAPE,
                   "aurppo_pack_records_f32: B=%d action_floats=%d (1..12)", B, action_floats);
    AURPPO_REQUIRE(aligned_to(rec4, 16) && aligned_to(rec64, 16), AURPPO_EINVAL, "aurppo_pack_records_f32: records not 16-byte aligned");
    hipLaunchKernelGGL(k_pack_rec64, dim3((B + 63) / 64), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(rec4),
                       actions, B, action_floats, reinterpret_cast<float4*>(rec64));
    AURPPO_LAUNCH_CHECK("k_pack_rec64");
    return AURPPO_OK;
}

extern "C" int aurppo_mlp_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                  const float* params, const int* layout_h, int n_params, float* actions, float* logp,
                                  float* value, void* stream) {
    AURPPO_REQUIRE(obs && params && layout_h && value, AURPPO_EINVAL, "aurppo_mlp_act_f32: null pointer");
    AURPPO_REQUIRE(!noise || (actions && logp), AURPPO_EINVAL, "aurppo_mlp_act_f32: sampling needs actions and logp outputs");
    AURPPO_REQUIRE(hidden == H, AURPPO_ESHAPE, "aurppo_mlp_act_f32: hidden_dim=%d (only %d is built)", hidden, H);
    AURPPO_REQUIRE(D >= 1 && D <= H, AURPPO_ESHAPE, "aurppo_mlp_act_f32: state_dim=%d must be 1..%d", D, H);
    AURPPO_REQUIRE(A >= 1 && A <= AP && (continuous || A >= 2), AURPPO_ESHAPE, "aurppo_mlp_act_f32: action_dim=%d", A);
    AURPPO_REQUIRE(N > 0 && n_params > 0, AURPPO_ESHAPE, "aurppo_mlp_act_f32: N=%d n_params=%d", N, n_params);
    ActArgs a;
    a.obs = obs; a.noise = noise; a.params = params; a.actions = actions; a.logp = logp; a.value = value;
    a.N = N; a.D = D; a.A = A; a.continuous = continuous ? 1 : 0;
    if (const int rc = fill_layout(a.L, layout_h, continuous, n_params, "aurppo_mlp_act_f32")) return rc;
    return launch_dyn_lds<k_mlp_act>("k_mlp_act", (N + R - 1) / R, kThreads, ActLds::bytes(true), ActLds::bytes(true), (hipStream_t)stream, a);
}
