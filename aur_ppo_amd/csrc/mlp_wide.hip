// K7w / K8w: the fused PPO minibatch step (as K7, mlp.hip / mlp2.hip) and the rollout step (as K8) for every MLP
// actor-critic the reference's CLI can ask for that is NOT the default 64-64 one: hidden_dim <= 128, num_layers 1..3,
// state_dim <= 128 (src/nets/nets.py:19-53 builds `num_layers` Tanh layers of `hidden_dim`; flags src/run_ppo.py:33,37).
// Same inputs, same outputs (per-workgroup gradient slabs + loss partials, folded by k_mlp_reduce, mlp_tail.hip; the optimizer
// step is K6b's), same fp32 MFMA arithmetic -- what differs is where things live, because at 128 x 3 neither the
// weights (2 x 192 KB) nor the weight-gradient accumulators (2 x 200 KB) of BOTH nets fit one CU:
//   * a workgroup (4 waves, one per SIMD) works on ONE net: actor and critic share nothing but the input rows and the
//     advantage statistics (the loss is a sum of an actor-only and a critic-only term), so even and odd workgroups
//     take the two nets of the same row tiles and write disjoint halves of the same slab;
//   * wave w owns the w-th 32-column block of every layer: its weight-gradient blocks (out-block 0..3, in-block w) of
//     every layer stay in registers over the whole launch (13 accumulators of 16 registers at 128 x 3: the 512-register
//     budget of one wave per SIMD is what makes that possible);
//   * the weights are not staged in LDS: a preparation kernel lays every hidden layer out once per launch in MFMA
//     B-operand order (forward: W^T blocks, backward: W blocks; zero-padded to 32-multiples), and a wave streams each
//     32x32 block with four 16-byte loads per lane from L2, one block ahead of the MFMA chain that consumes it;
//   * activations live in LDS ([32 rows][129]); dZ_l overwrites H_l in place (a wave only ever reads its own column
//     block of H_l once dZ_l is being formed), so a layer costs one 16.5 KB buffer.
// When nothing is wider than 64 (two column blocks) a workgroup carries BOTH nets instead -- waves 0,1 the actor's
// column blocks, waves 2,3 the critic's -- in a geometry (row stride 65, 256 registers) that fits a CU twice, so two
// independent workgroups overlap each other's epilogues and barriers the way k_mlp_step2's two tile sets do.
// Tiles are handed out by a counter.  Measured against the per-op path it replaces in DESIGN section 4.3c.
// This file: the fp32-MFMA kernels, the rollout kernel, the host side and the C entries.  The default step of the shapes wider than 64,
// k_mlpw3_step on the bf16 matrix pipe, is mlp_wide3.hip; what the two share (argument block, workspace, common passages) is mlp_wide.h.
#include <stdlib.h>

#pragma clang fp contract(fast)
#include "mlp_wide.h"
#include "mlp_tail.h"

using namespace aurppo_mlp;

namespace {

// stats[b] = partial (sum, sum of squares) of the minibatch's advantages; wop = every hidden layer of both nets in
// operand order (mlp_common.h: op_at / op_index), walked entry by entry so that the padding is zero without a clearing pass.
__global__ __launch_bounds__(256) void k_mlpw_prep(const float* __restrict__ params, WideLayout L, int NL, int D, int Hd,
                                                   float* __restrict__ wop, const float4* __restrict__ rec, int rec_stride,
                                                   const int32_t* __restrict__ idx, int M, double (*__restrict__ stats)[2],
                                                   int n_stat_blocks, unsigned* __restrict__ tile_counter) {
    __shared__ double sc[2][4];
    if (prep_stats(sc, rec, rec_stride, idx, M, stats, n_stat_blocks, tile_counter)) return;
    const int b = blockIdx.x - n_stat_blocks, nb = gridDim.x - n_stat_blocks;
    for (int e = b * 256 + threadIdx.x; e < kOpFloats; e += nb * 256) {
        // (the entry number's own fields: e = op_at(n, l, dir, hi, kb, lane, m))
        const int m = e & 15, lane = (e >> 4) & 63, blk = (e >> 10) & 15, dir = (e >> 14) & 1, nl = e >> 15;
        const int n = nl / MAXL, l = nl - n * MAXL;
        if (l >= NL || (dir == 1 && l == 0)) continue;
        const int in_dim = l == 0 ? D : Hd;
        const float* W = params + L.w[n][l];
        const int hi = blk >> 2, kb = blk & 3;
        int row, col;
        if (dir == 0) {
            row = op_j(hi, lane);
            col = op_k(kb, lane, m);
        } else {
            row = op_k(kb, lane, m);
            col = op_j(hi, lane);
        }
        wop[e] = (row < Hd && col < in_dim) ? W[row * in_dim + col] : 0.0f;
    }
}
static_assert(op_at(0, 0, 0, 0, 0, 0, 1) == 1 && op_at(0, 0, 0, 0, 0, 1, 0) == 16 && op_at(0, 0, 0, 0, 1, 0, 0) == (1 << 10) &&
              op_at(0, 0, 0, 1, 0, 0, 0) == (4 << 10) && op_at(0, 0, 1, 0, 0, 0, 0) == (1 << 14) && op_at(0, 1, 0, 0, 0, 0, 0) == (1 << 15) &&
              op_at(1, 0, 0, 0, 0, 0, 0) == (MAXL << 15), "k_mlpw_prep reads an entry's fields out of its number");

// this lane's 16 steps of block (hi, kb) of copy (net, l, dir) = wop + op_at(net, l, dir, hi, kb, lane, 0), taken in three pointer steps:
// the step kernels' address code was tuned in this form, and one combined offset compiles to other instructions in all of them
__device__ __forceinline__ const float* op_block(const float* wop, int net, int l, int dir, int hi, int kb, int lane) {
    return wop + op_copy(net, l, dir) + op_entry(hi, kb, 0, 0) + op_entry(0, 0, lane, 0);
}

__device__ __forceinline__ void load_b(float (&b)[16], const float* p) {
    const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float4 v = q[u];
        b[4 * u + 0] = v.x; b[4 * u + 1] = v.y; b[4 * u + 2] = v.z; b[4 * u + 3] = v.w;
    }
}

// acc += A(32 x 32) * B(32 x 32): A from LDS through a_at(i, k), B already in registers (operand order)
template <class FA>
__device__ __forceinline__ void mma_breg(f32x16& acc, FA a_at, const float (&b)[16], int lane) {
    const int ij = lane & 31, kk = lane >> 5;
    float av[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) av[m] = a_at(ij, 2 * m + kk);
#pragma unroll
    for (int m = 0; m < 16; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], b[m], acc, 0, 0, 0);
}

// One output block of a layer: acc = sum over nkb in-blocks of In[:, kb] * Wop[block (hi, kb)], the weight blocks
// streamed one ahead.  In: [R][LDW] in LDS.
// LOAD_FIRST = false: `early` already holds (or is loading) the layer's first block -- the caller issued that load a phase
// early, behind work that does not need it, so its L2 latency is not on the chain (EARLY below; not with three 128-wide
// layers, whose accumulators leave no registers to hold a block across a phase).
template <bool LOAD_FIRST, int LD_>
__device__ __forceinline__ f32x16 stream_layer(const float* In, const float* wop, int net, int l, int dir, int hi, int nkb,
                                               int lane, float (&early)[16]) {
    f32x16 acc = zero16();
    float bq[2][16];
    if (LOAD_FIRST) {
        load_b(bq[0], op_block(wop, net, l, dir, hi, 0, lane));
    } else {
#pragma unroll
        for (int m = 0; m < 16; ++m) bq[0][m] = early[m];
    }
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        if (kb < nkb) {
            if (kb + 1 < nkb) load_b(bq[(kb + 1) & 1], op_block(wop, net, l, dir, hi, kb + 1, lane));
            mma_breg(acc, [&](int i, int k) { return In[i * LD_ + kb * 32 + k]; }, bq[kb & 1], lane);
        }
    }
    return acc;
}

struct WideLds {
    float* sX;            // [R][LDW]
    float* sH[MAXL];      // [R][LDW] each; dZ_l overwrites H_l in the backward pass
    float* sW3;           // [AP][LDW] head weights of this net, rows >= out_dim zero
    float* sOut;          // [R][LDO] head outputs, then their gradients
    float* sAct;          // [R][LDO]
    float* sDls;          // [R][LDO] per-sample d logstd terms (actor)
    float* sB;            // [MAXL][HPW] hidden biases, zero beyond Hd
    float* sB3;           // [AP]
    float* sLs;           // [AP]
    float* sIvar;         // [AP]  1 / sigma^2 (step) | sigma (act)
    float4* sRec;         // [R]
    int* sSrc;            // [R]
    int* sIdx;            // [2][R]
};

// [sX][per-net block x nslots][sAct sDls sLs sIvar sRec sSrc sIdx]: one net per workgroup, or both (nslots = 2) when the
// layers are at most 64 wide -- see k_mlpw_step.  NARROW (that case): row stride 65 and 64 bias slots per layer, so that two
// such workgroups fit one CU's 160 KB.
template <bool NARROW> struct Geo {
    static constexpr int LD = NARROW ? 65 : LDW;      // row stride of an activation matrix (odd either way)
    static constexpr int HP = NARROW ? 64 : HPW;      // bias slots per layer
};
template <bool NARROW, int NL>
constexpr int net_floats() { return NL * R * Geo<NARROW>::LD + AP * Geo<NARROW>::LD + R * LDO + MAXL * Geo<NARROW>::HP + AP; }
constexpr int kTailFloats = 2 * R * LDO + 2 * AP;
template <bool NARROW, int NL>
__device__ __forceinline__ WideLds carve(float* lds, int slot, int nslots) {
    constexpr int LD_ = Geo<NARROW>::LD;
    WideLds s;
    s.sX = lds;
    float* nb = lds + R * LD_ + slot * net_floats<NARROW, NL>();
    for (int l = 0; l < MAXL; ++l) s.sH[l] = nb + (l < NL ? l : 0) * R * LD_;
    s.sW3 = nb + NL * R * LD_;
    s.sOut = s.sW3 + AP * LD_;
    s.sB = s.sOut + R * LDO;
    s.sB3 = s.sB + MAXL * Geo<NARROW>::HP;
    float* tail = lds + R * LD_ + nslots * net_floats<NARROW, NL>();
    s.sAct = tail;
    s.sDls = s.sAct + R * LDO;
    s.sLs = s.sDls + R * LDO;
    s.sIvar = s.sLs + AP;
    s.sRec = reinterpret_cast<float4*>(s.sIvar + AP);   // every term above is a multiple of 4 floats
    s.sSrc = reinterpret_cast<int*>(s.sRec + R);
    s.sIdx = s.sSrc + R;
    return s;
}
static_assert((R * LDW) % 4 == 0 && (R * 65) % 4 == 0 && net_floats<false, 1>() % 4 == 0 && net_floats<false, 2>() % 4 == 0 &&
              net_floats<false, 3>() % 4 == 0 && net_floats<true, 1>() % 4 == 0 && net_floats<true, 2>() % 4 == 0 &&
              net_floats<true, 3>() % 4 == 0 && kTailFloats % 4 == 0, "sRec must be 16-B aligned");
template <bool NARROW, int NL>
constexpr size_t wide_lds_bytes(int nslots) {
    return sizeof(float) * (size_t)(R * Geo<NARROW>::LD + nslots * net_floats<NARROW, NL>() + kTailFloats + 4 * R + R + 2 * R);
}
static_assert(2 * (wide_lds_bytes<true, 3>(2) + 1024) <= 160 * 1024, "two both-net workgroups of a <= 64-wide policy must fit one CU's LDS");

// weights that stay in LDS: the head, every bias, log-std
template <int NL, bool NARROW>
__device__ __forceinline__ void stage_small(const WideArgs& a, const WideLds& s, int net, bool act_mode) {
    constexpr int LD_ = Geo<NARROW>::LD, HP_ = Geo<NARROW>::HP;
    const int tid = threadIdx.x, Hd = a.Hd, out_dim = net == 0 ? a.A : 1;
    for (int e = tid; e < R * LD_; e += kThreads) s.sX[e] = 0.0f;
    for (int e = tid; e < AP * LD_; e += kThreads) {
        const int o = e / LD_, i = e - o * LD_;
        s.sW3[e] = (o < out_dim && i < Hd) ? a.params[a.L.w[net][NL] + o * Hd + i] : 0.0f;
    }
    stage_biases<NL, HP_>(a, net, s.sB, s.sB3, s.sLs, s.sIvar, act_mode);
    for (int e = tid; e < R * LDO; e += kThreads) s.sDls[e] = 0.0f;
}

// forward pass of one net over the tile in sX: H_1 .. H_NL, then the head into sOut (+ bias)
template <int NL, bool EARLY, bool NARROW>
__device__ __forceinline__ void forward_tile(const WideArgs& a, const WideLds& s, int net, int cb, int HB, int DB,
                                             float (&early)[16]) {
    constexpr int LD_ = Geo<NARROW>::LD, HP_ = Geo<NARROW>::HP;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (cb < HB) {
            const float* In = l == 0 ? s.sX : s.sH[l - 1];
            const f32x16 acc = stream_layer<!EARLY, LD_>(In, a.wop, net, l, 0, cb, l == 0 ? DB : HB, lane, early);
            if (EARLY && l + 1 < NL) load_b(early, op_block(a.wop, net, l + 1, 0, cb, 0, lane));   // behind the epilogue and the barrier
            const int col = cb * 32 + (lane & 31);
            const float bias = s.sB[l * HP_ + col];
            float* Hl = s.sH[l];
#pragma unroll
            for (int e = 0; e < 16; ++e) Hl[acc_row(e, lane) * LD_ + col] = tanh_fast(acc[e] + bias);
        }
        __syncthreads();
    }
    if (cb < 2) {   // head: 16 rows per wave as one 16x16 tile, K = HB blocks of 32
        const float* Hin = s.sH[NL - 1] + cb * 16 * LD_;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
            if (kb < HB)
                acc += mma16<32>([&](int i, int k) { return Hin[i * LD_ + kb * 32 + k]; },
                                 [&](int k, int j) { return s.sW3[j * LD_ + kb * 32 + k]; });
        const int col = lane & 15;
        const float bias = s.sB3[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) s.sOut[(cb * 16 + 4 * (lane >> 4) + e) * LDO + col] = acc[e] + bias;
    }
    __syncthreads();
}

// DUAL = false: a workgroup is one net (blockIdx & 1), wave w owns column block w (layers up to 128 wide).
// DUAL = true (layers and state at most 64 wide, i.e. two column blocks): a workgroup is BOTH nets of its tiles -- waves
// 0,1 the actor's two column blocks, waves 2,3 the critic's -- so no wave idles and a tile's rows are fetched once.
template <int NL, bool DUAL>
__global__ __launch_bounds__(256, DUAL ? 2 : 1) void k_mlpw_step(const WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double s_red[2][kThreads / kWave];
    __shared__ float s_mean, s_std;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int net = DUAL ? (w >> 1) : (int)(blockIdx.x & 1), cb = DUAL ? (w & 1) : w;
    const int pair = DUAL ? (int)blockIdx.x : (int)(blockIdx.x >> 1);
    constexpr int LD_ = Geo<DUAL>::LD;
    constexpr int XS = DUAL ? 8 : 16;    // staging slots per thread: columns (tid & 7) + 8u cover 64 or 128 state floats
    const WideLds s = carve<DUAL, NL>(lds, DUAL ? net : 0, DUAL ? 2 : 1);
    const int hw = DUAL ? 1 : 3;          // the actor wave that also forms the head-side column sums
    const int lrow = DUAL ? (tid & 127) : tid;   // loss lanes: the first 32 lanes of each net's first wave
    const int D = a.D, A = a.A, Hd = a.Hd;
    const int HB = (Hd + 31) >> 5, DB = (D + 31) >> 5;
    const int AW = a.continuous ? A : 1;
    const int out_dim = net == 0 ? A : 1;
    const bool own_out = NL < 3 && DB < HB;   // (not with three layers: no registers for a second code path)
    constexpr bool EARLY = DUAL ? NL == 1 : NL < 3;   // holding a weight block across a phase costs 16 registers
    constexpr int CHW = (NL == 3 || DUAL) ? 4 : 8;   // operand read-ahead of the LDS-fed chains: three layers of accumulators leave fewer registers

    if (DUAL) {
        stage_small<NL, DUAL>(a, carve<DUAL, NL>(lds, 0, 2), 0, false);
        stage_small<NL, DUAL>(a, carve<DUAL, NL>(lds, 1, 2), 1, false);
    } else {
        stage_small<NL, DUAL>(a, s, net, false);
    }
    fold_adv_stats(a, s_red, s_mean, s_std);
    __syncthreads();
    const float mean = s_mean, denom = s_std + 1e-8f;
    const float invM = 1.0f / (float)a.h.M;
    const float g_ent = -a.h.ent_coef * invM;

    // persistent accumulators: dW_l blocks (out-block ob, in-block w), head block (rows < AP, in-block w), bias columns
    constexpr int OBN = DUAL ? 2 : 4;   // out-blocks a layer can have
    f32x16 gW[NL][OBN];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int ob = 0; ob < OBN; ++ob) gW[l][ob] = zero16();
    f32x16 gW3 = zero16();
    float gb[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) gb[l] = 0.0f;
    double l_a = 0, l_b = 0, l_c = 0, l_d = 0, l_e = 0;   // actor: pg, ent, okl, kl, cf; critic: vl in l_a
    float g_b3c = 0.0f, g_head = 0.0f;

    const int n_tiles = (a.h.M + R - 1) / R;
    // staging slots: 8 threads per row, columns (tid & 7) + 8u
    const int x_r = tid >> 3, x_c0 = tid & 7;
    float xr[XS], ar[2];
    unsigned xok = 0u;               // bit u: xr[u] is real; bit 16 + u: ar[u] (the zeroing waits until the tile lands)
    float4 p_rec = make_float4(0.f, 0.f, 0.f, 0.f);
    int p_src = -1, n_raw = 0;
    bool n_ok = false;
    const ActRows arows = act_rows(a, AW);
    // (every load unconditional, nothing computed from its result here: mlp_wide.h, k_mlpw3_step's lesson)
    auto prefetch = [&](const int* sidx) {
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int src = sidx[tq >> 3];
        xok = 0u;
#pragma unroll
        for (int u = 0; u < XS; ++u) {
            const int c = (tq & 7) + 8 * u;
            const bool ok = src >= 0 && c < D;
            const unsigned row = ok ? (unsigned)src : 0u, col = ok ? (unsigned)c : 0u;
            xr[u] = a.obs[(size_t)row * (unsigned)D + col];
            xok |= ok ? (1u << u) : 0u;
        }
        if (DUAL || net == 0) prefetch_actions(sidx, tq, arows, AW, xok, [&](int u, const float* p) { ar[u] = *p; });
        prefetch_record(a, sidx, tq, p_src, p_rec);
    };
    // the tile queue (mlp_wide.h)
    __shared__ int s_tile[4];
    const TileQueue queue = {a.tile_counter + (DUAL ? 0 : net), a.static_tiles != 0, pair, DUAL ? (int)gridDim.x : (int)(gridDim.x >> 1)};
    if (tid == 0) tile_queue_start(queue, s_tile);
    __syncthreads();
    if (tid < R) {
        s.sIdx[tid] = load_idx(a, n_tiles, s_tile[0]);
        s.sIdx[R + tid] = load_idx(a, n_tiles, s_tile[1]);
    }
    __syncthreads();
    prefetch(s.sIdx);
    prefetch_idx(a, n_tiles, s_tile[2], n_ok, n_raw);
    for (int it = 0;; ++it) {
        const int tile = s_tile[it & 3];
        if (tile >= n_tiles) break;
        const int tile3 = s_tile[(it + 3) & 3];
        // ---- land the prefetched tile, start fetching the next one
        float early[16];
        if (EARLY && cb < HB) load_b(early, op_block(a.wop, net, 0, 0, cb, 0, lane));   // layer 1's first weight block, behind the landing
#pragma unroll
        for (int u = 0; u < XS; ++u) {
            const int c = x_c0 + 8 * u;
            if (c < D) s.sX[x_r * LD_ + c] = ((xok >> u) & 1u) ? xr[u] : 0.0f;
        }
        if (DUAL || net == 0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = tid + u * kThreads;
                s.sAct[(e >> 4) * LDO + (e & 15)] = ((xok >> (16 + u)) & 1u) ? ar[u] : 0.0f;
            }
        }
        if (tid < R) {
            s.sSrc[tid] = p_src;
            s.sRec[tid] = p_rec;
            s.sIdx[(it & 1) * R + tid] = n_ok ? n_raw : -1;
        }
        __syncthreads();
        // the next tile's rows are fetched behind this tile's math -- except with three layers, whose accumulators leave
        // no registers to hold them that long: there they are fetched at the end of the tile (latency exposed, ~5 %)
        if (NL < 3) prefetch(s.sIdx + ((it + 1) & 1) * R);
        prefetch_idx(a, n_tiles, tile3, n_ok, n_raw);

        forward_tile<NL, EARLY, DUAL>(a, s, net, cb, HB, DB, early);
        // the tile after the three already known: asked for here, where this wave has no loads queued behind the atomic
        // (returns are in order), stored in s_tile at the end of the tile
        int tile4 = 0;
        if (tid == 0) tile4 = tile_queue_next(queue, tile);

        // ---- loss lanes (one per row): this net's half of the PPO terms; head outputs become their gradients
        if (lrow < R) {
            float* out = s.sOut + lrow * LDO;
            if (s.sSrc[lrow] >= 0) {
                const float4 rc = s.sRec[lrow];
                if (net == 1) {
                    const PpoSample t = ppo_sample(rc.x, rc.x, rc.y, out[0], rc.w, rc.z, mean, denom, invM, a.h);
                    l_a += t.vl;
                    out[0] = t.g_v;
                    g_b3c += t.g_v;
                } else if (a.continuous) {
                    const float* act = s.sAct + lrow * LDO;
                    float logp = 0.0f, ent = 0.0f;
                    for (int k = 0; k < A; ++k) {
                        const float ls = s.sLs[k];
                        const float zk = act[k] - out[k];
                        logp += gauss_logp_ivar(zk, s.sIvar[k], ls);
                        ent += gauss_ent(ls);
                    }
                    const PpoSample t = ppo_sample(logp, rc.x, rc.y, rc.w, rc.w, rc.z, mean, denom, invM, a.h);
                    l_a += t.pg; l_b += ent; l_c += t.okl; l_d += t.kl; l_e += t.cf;
                    for (int k = 0; k < A; ++k) {
                        const float zk = act[k] - out[k];
                        out[k] = gauss_dmu(t.g_logp, zk, s.sIvar[k]);
                        s.sDls[lrow * LDO + k] = gauss_dls(t.g_logp, zk, s.sIvar[k], g_ent);
                    }
                } else {
                    const float* act = s.sAct + lrow * LDO;
                    const float lse = cat_lse(out, A);
                    const int ai = (int)act[0];
                    float logp = 0.0f, ent = 0.0f;
                    for (int k = 0; k < A; ++k) {
                        const float lpk = out[k] - lse;
                        ent -= expf(lpk) * lpk;
                        if (k == ai) logp = lpk;
                    }
                    const PpoSample t = ppo_sample(logp, rc.x, rc.y, rc.w, rc.w, rc.z, mean, denom, invM, a.h);
                    l_a += t.pg; l_b += ent; l_c += t.okl; l_d += t.kl; l_e += t.cf;
                    for (int k = 0; k < A; ++k) {
                        const float lpk = out[k] - lse;
                        const float pk = expf(lpk);
                        out[k] = cat_dlogit(t.g_logp, k == ai, pk, lpk, ent, g_ent);
                    }
                }
            } else {
                for (int k = 0; k < AP; ++k) out[k] = s.sDls[lrow * LDO + k] = 0.0f;
            }
        }
        __syncthreads();

        // ---- head backward: column sums (d b3, d logstd), dH_NL -> dZ_NL (in place), dW3
        if (net == 0 && w == hw && lane < 2 * AP) g_head += head_colsum(s.sOut, s.sDls, lane);
        if (cb < HB) {
            float* HL = s.sH[NL - 1];
            f32x16 acc = zero16();
            mma32<AP>(acc, [&](int i, int k) { return s.sOut[i * LDO + k]; },
                      [&](int k, int j) { return s.sW3[k * LD_ + cb * 32 + j]; });
            mma32<R, CHW>(gW3, [&](int i, int k) { return i < AP ? s.sOut[k * LDO + i] : 0.0f; },
                          [&](int k, int j) { return HL[k * LD_ + cb * 32 + j]; }, lane);
            const int col = cb * 32 + (lane & 31);
            float colsum = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float* hp = HL + acc_row(e, lane) * LD_ + col;
                const float h = *hp;
                const float dz = acc[e] * (1.0f - h * h);
                colsum += dz;
                *hp = dz;
            }
            colsum += __shfl_xor(colsum, 32, kWave);
            gb[NL - 1] += colsum;
        }
        __syncthreads();
        // ---- hidden layers, top down: dW_l, dH_{l-1} -> dZ_{l-1} (in place)
#pragma unroll
        for (int l = NL - 1; l >= 1; --l) {
            if (cb < HB) {
                const float* dZ = s.sH[l];
                float* Hp = s.sH[l - 1];
                if (EARLY) load_b(early, op_block(a.wop, net, l, 1, cb, 0, lane));   // dH's first weight block, behind the dW chains
#pragma unroll
                for (int ob = 0; ob < OBN; ++ob)
                    if (ob < HB)
                        mma32<R, CHW>(gW[l][ob], [&](int i, int k) { return dZ[k * LD_ + ob * 32 + i]; },
                                      [&](int k, int j) { return Hp[k * LD_ + cb * 32 + j]; }, lane);
                const f32x16 acc = stream_layer<!EARLY, LD_>(dZ, a.wop, net, l, 1, cb, HB, lane, early);
                const int col = cb * 32 + (lane & 31);
                float colsum = 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float* hp = Hp + acc_row(e, lane) * LD_ + col;
                    const float h = *hp;
                    const float dz = acc[e] * (1.0f - h * h);
                    colsum += dz;
                    *hp = dz;
                }
                colsum += __shfl_xor(colsum, 32, kWave);
                gb[l - 1] += colsum;
            }
            __syncthreads();
        }
        // ---- dW_1: a wave owns the state's in-block cb and walks the out-blocks, as for the other layers -- unless the
        // state is narrower than the layer (DB < HB), where owning OUT-block cb and walking the in-blocks keeps every
        // wave busy (gW[0][k] is then block (cb, k) instead of (k, cb))
        if (own_out) {
            if (cb < HB) {
                const float* dZ = s.sH[0];
#pragma unroll
                for (int ib = 0; ib < OBN; ++ib)
                    if (ib < DB)
                        mma32<R, CHW>(gW[0][ib], [&](int i, int k) { return dZ[k * LD_ + cb * 32 + i]; },
                                      [&](int k, int j) { return s.sX[k * LD_ + ib * 32 + j]; }, lane);
            }
        } else if (cb < DB) {
            const float* dZ = s.sH[0];
#pragma unroll
            for (int ob = 0; ob < OBN; ++ob)
                if (ob < HB)
                    mma32<R, CHW>(gW[0][ob], [&](int i, int k) { return dZ[k * LD_ + ob * 32 + i]; },
                                  [&](int k, int j) { return s.sX[k * LD_ + cb * 32 + j]; }, lane);
        }
        if (NL >= 3) prefetch(s.sIdx + ((it + 1) & 1) * R);
        if (tid == 0) s_tile[it & 3] = tile4;               // everyone read this slot at the top of the tile
        __syncthreads();
    }

    // ---- this workgroup's half of the pair's slab
    float* slab = a.slabs + (size_t)pair * a.L.n_params;
    {
        const int col = cb * 32 + (lane & 31);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int in_dim = l == 0 ? D : Hd;
#pragma unroll
            for (int ob = 0; ob < OBN; ++ob) {
                if (l == 0 && own_out) {       // gW[0][ob] = block (out cb, in ob)
                    const int c0 = ob * 32 + (lane & 31);
                    if (ob < DB && cb < HB && c0 < D) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int o = cb * 32 + acc_row(e, lane);
                            if (o < Hd) slab[a.L.w[net][0] + o * D + c0] = gW[0][ob][e];
                        }
                    }
                } else if (ob < HB && col < in_dim) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int o = ob * 32 + acc_row(e, lane);
                        if (o < Hd) slab[a.L.w[net][l] + o * in_dim + col] = gW[l][ob][e];
                    }
                }
            }
            if (lane < 32 && col < Hd) slab[a.L.b[net][l] + col] = gb[l];
        }
        if (col < Hd) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = acc_row(e, lane);
                if (o < out_dim) slab[a.L.w[net][NL] + o * Hd + col] = gW3[e];
            }
        }
    }
    if (net == 0 && w == hw) slab_head_sums<NL>(slab, a, lane, g_head);
    if (cb == 0) {
        float c = lane < R ? g_b3c : 0.0f;
        double v5[5] = {l_a, l_b, l_c, l_d, l_e};
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) c += __shfl_down(c, off, kWave);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double x = lane < R ? v5[q] : 0.0;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) x += __shfl_down(x, off, kWave);
            v5[q] = x;
        }
        if (lane == 0) loss_record<NL>(a, slab, pair, net, v5, c, mean, s_std);
    }
}

// K8w: policy.evaluate(next_obs) under no_grad + the three buffer row stores (src/ppo.py:103-108), or value only
// (noise == nullptr, src/ppo.py:161).  Workgroup = (row tile, net).
template <int NL>
__global__ __launch_bounds__(256) void k_mlpw_act(const WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const WideLds s = carve<false, NL>(lds, 0, 1);
    const int tid = threadIdx.x;
    const int net = a.net_base + (int)(blockIdx.x % a.net_count), row0 = (int)(blockIdx.x / a.net_count) * R;
    const int D = a.D, A = a.A, HB = (a.Hd + 31) >> 5, DB = (D + 31) >> 5;
    stage_small<NL, false>(a, s, net, true);
    __syncthreads();
    {
        const int r = tid >> 3, n = row0 + r;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = (tid & 7) + 8 * u;
            if (c < D) s.sX[r * LDW + c] = n < a.N ? a.obs[(size_t)n * D + c] : 0.0f;
        }
    }
    __syncthreads();
    float early[16];
    if ((tid >> 6) < HB) load_b(early, op_block(a.wop, net, 0, 0, tid >> 6, 0, tid & 63));
    forward_tile<NL, true, false>(a, s, net, tid >> 6, HB, DB, early);
    if (tid >= R || row0 + tid >= a.N) return;
    const int n = row0 + tid;
    const float* mu = s.sOut + tid * LDO;
    if (net == 1) {
        a.out_value[n] = mu[0];
        return;
    }
    if (!a.noise) return;
    if (a.continuous) {
        float lp = 0.0f;
        for (int k = 0; k < A; ++k)      // (sIvar holds exp(logstd) here: stage_small's last argument)
            lp += gauss_sample(mu[k], s.sIvar[k], s.sLs[k], a.noise[(size_t)n * A + k], a.out_actions[(size_t)n * A + k]);
        a.out_logp[n] = lp;
    } else {
        const float lse = cat_lse(mu, A);
        float lp;
        a.out_actions[n] = (float)cat_sample(mu, A, lse, a.noise[n], lp);
        a.out_logp[n] = lp;
    }
}

// slabs a launch can write: two both-net workgroups per CU for the narrow shapes (small n_params), one pair per two CUs otherwise
int wide_slab_cap(int hidden, int D) { return (hidden <= 64 && D <= 64) ? kMaxSlabs : kMaxGrid / 2; }
// The argument block as the step and the rollout entries start it: input rows, parameters, the net's shape and its layout.
// layout_h: for net in (actor, critic): w_0, b_0, ..., w_NL, b_NL (layer NL = head); then logstd
int wide_args(WideArgs& a, const float* obs, const float* params, int D, int A, int continuous, int hidden, int NL, const int* layout_h,
              int n_params, const char* who) {
    a = {};
    a.obs = obs; a.params = params;
    a.D = D; a.A = A; a.Hd = hidden; a.continuous = continuous ? 1 : 0;
    WideLayout& L = a.L;
    const int per = 2 * (NL + 1);
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l <= NL; ++l) {
            L.w[n][l] = layout_h[n * per + 2 * l];
            L.b[n][l] = layout_h[n * per + 2 * l + 1];
        }
    L.logstd = continuous ? layout_h[2 * per] : 0;
    L.n_params = n_params;
    for (int k = 0; k < 2 * per + (continuous ? 1 : 0); ++k)
        AURPPO_REQUIRE(layout_h[k] >= 0 && layout_h[k] < n_params, AURPPO_ESHAPE, "%s: layout[%d]=%d", who, k, layout_h[k]);
    return AURPPO_OK;
}

int check_shape(int D, int A, int continuous, int hidden, int num_layers, const char* who) {
    AURPPO_REQUIRE(hidden >= 1 && hidden <= HPW, AURPPO_ESHAPE, "%s: hidden_dim=%d must be 1..%d", who, hidden, HPW);
    AURPPO_REQUIRE(num_layers >= 1 && num_layers <= MAXL, AURPPO_ESHAPE, "%s: num_layers=%d must be 1..%d", who, num_layers, MAXL);
    AURPPO_REQUIRE(D >= 1 && D <= HPW, AURPPO_ESHAPE, "%s: state_dim=%d must be 1..%d", who, D, HPW);
    AURPPO_REQUIRE(A >= 1 && A <= AP && (continuous || A >= 2), AURPPO_ESHAPE,
                   "%s: action_dim=%d must be 1..%d (>= 2 logits for a Categorical head)", who, A, AP);
    return AURPPO_OK;
}

}  // namespace

extern "C" size_t aurppo_mlp_wide_workspace_bytes(int n_params, int hidden, int state_dim) {
    // the slab region is sized from the shape (512 slabs of a narrow policy's few parameters, 128 of a wide one's many: 52 MB
    // instead of 207 MB at 3 x 128 over 128 state floats); n_params = 0: the operand copies alone, all K8w needs
    return wide_ws(nullptr, n_params > 0 ? n_params : 0, wide_slab_cap(hidden, state_dim)).bytes;
}

// Which kernel aurppo_mlp_wide_ppo_*_f32 launches for a net shape: 1 = k_mlpw_step<., true> (both nets per workgroup, fp32 MFMA:
// nothing wider than 64), 2 = k_mlpw_step<., false> (one net per workgroup, fp32 MFMA), 3 = k_mlpw3_step (one net per workgroup,
// bf16 MFMA over three-way splits -- the default for the wider shapes; AURPPO_K7W_VARIANT=2 selects 2).
extern "C" int aurppo_k7w_kernel(int hidden, int state_dim) {
    if (hidden <= 64 && state_dim <= 64) return 1;
    return aurppo_knobs().k7w_variant == 3 ? 3 : 2;
}

// The prepare pass: the operand copies the kernel behind it streams (bf3k: k_mlpw3_step's bf16 planes), and in front of them sb
// workgroups of advantage partial sums (0: K8w, which needs neither them nor the counters)
static int wide_prep(bool bf3k, const WideArgs& a, int num_layers, int M, int sb, const WideWs& wv, hipStream_t s) {
    double* const stats = sb ? wv.stats : nullptr;
    unsigned* const tile_counter = sb ? wv.tile_counter : nullptr;
    if (bf3k) return launch_mlpw3_prep(a, num_layers, M, sb, stats, tile_counter, wv.wop3, s);
    hipLaunchKernelGGL(k_mlpw_prep, dim3(sb + 96), dim3(256), 0, s, a.params, a.L, num_layers, a.D, a.Hd, wv.wop, a.rec, a.rec_stride, a.idx, M,
                       reinterpret_cast<double (*)[2]>(stats), sb, tile_counter);
    AURPPO_LAUNCH_CHECK("k_mlpw_prep");
    return AURPPO_OK;
}
// k_mlpw_step: both nets per workgroup (dual) or one
static int launch_mlpw_step(const WideArgs& a, int num_layers, bool dual, int grid, hipStream_t s) {
    return wide_with_nl(num_layers, [&](auto n) {
        constexpr int NL = decltype(n)::value;
        if (dual) return wide_launch<k_mlpw_step<NL, true>>("k_mlpw_step", grid, wide_lds_bytes<true, NL>(2), s, a);
        return wide_launch<k_mlpw_step<NL, false>>("k_mlpw_step", grid, wide_lds_bytes<false, NL>(1), s, a);
    });
}
static int wide_step_impl(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A,
                          int continuous, int hidden, int num_layers, const float* params, const int* layout_h, int n_params,
                          float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                          float* out_scalars, void* workspace, void* stream, void* ev_begin, void* ev_end, const MlpTail* tail,
                          const char* who) {
    int rc = check_step_args(who, obs && rec && idx && params && layout_h && grads && out_scalars && workspace, actions, continuous, A, M,
                             n_params, vloss_mode, [&] { return check_shape(D, A, continuous, hidden, num_layers, who); });
    if (rc != AURPPO_OK) return rc;
    AURPPO_REQUIRE(aligned_to(workspace, 64) && aligned_to(rec, 16), AURPPO_EINVAL, "%s: workspace not 64-byte / rec not 16-byte aligned", who);
    WideArgs a;
    rc = wide_args(a, obs, params, D, A, continuous, hidden, num_layers, layout_h, n_params, who);
    if (rc != AURPPO_OK) return rc;
    a.actions = actions; a.rec = reinterpret_cast<const float4*>(rec); a.rec_stride = actions ? 1 : 4;
    a.idx = idx;
    a.h = make_hyper(M, clip, ent_coef, vf_coef, norm_adv, vloss_mode);
    const WideWs wv = wide_ws(workspace, n_params, wide_slab_cap(hidden, D));
    a.stats = wv.stats; a.loss_part = wv.loss_part; a.wop = wv.wop; a.slabs = wv.slabs; a.tile_counter = wv.tile_counter;
    a.wop3 = wv.wop3;
    hipStream_t s = (hipStream_t)stream;
    const int sb = stat_blocks_for(M);
    a.n_stat_blocks = sb;
    // layers and state at most two 32-column blocks wide: one workgroup carries both nets (k_mlpw_step<., true>, fp32 MFMA);
    // anything wider: one net per workgroup on the bf16 pipe (k_mlpw3_step; AURPPO_K7W_VARIANT=2 keeps the fp32-MFMA k_mlpw_step)
    const bool dual = hidden <= 64 && D <= 64;
    const AurppoKnobs& knobs = aurppo_knobs();
    const bool bf3k = !dual && knobs.k7w_variant == 3;
    if (!(tail && tail->chained)) {   // otherwise the previous chained call's optimizer launch has left all of this
        rc = wide_prep(bf3k, a, num_layers, M, sb, wv, s);
        if (rc != AURPPO_OK) return rc;
    }
    const int cus = aurppo_cu_count(kMaxGrid);
    if (cus < 0) return cus;
    const int n_tiles = (M + R - 1) / R;
    // 8 CUs left to the side stream's shuffle kernels, as K7; a both-net workgroup is built to share its CU with a second one
    a.static_tiles = knobs.static_tiles ? 1 : 0;
    int pairs = dual ? 2 * (cus - spare_cus()) : (cus - spare_cus()) / 2;
    if (pairs > (dual ? kMaxSlabs : kMaxGrid / 2)) pairs = dual ? kMaxSlabs : kMaxGrid / 2;
    if (pairs > n_tiles) pairs = n_tiles;
    if (pairs < 1) pairs = 1;
    if (ev_begin) AURPPO_HIP_TRY(hipEventRecord((hipEvent_t)ev_begin, s));
    const int grid = dual ? pairs : 2 * pairs;
    rc = bf3k ? launch_mlpw3_step(a, num_layers, grid, s) : launch_mlpw_step(a, num_layers, dual, grid, s);
    if (rc != AURPPO_OK) return rc;
    if (ev_end) AURPPO_HIP_TRY(hipEventRecord((hipEvent_t)ev_end, s));
    // (with a tail the reduce clears the tile counters for the launch that follows: the next chained call has no prepare pass to do it)
    TailWork w = {};
    w.slabs = wv.slabs; w.slab_strided = false; w.loss_part = wv.loss_part; w.n_slabs = pairs; w.n_params = n_params; w.h = a.h;
    w.grads = grads; w.out_scalars = out_scalars; w.sq_part = wv.sq_part; w.counters = wv.tile_counter;
    w.rec = a.rec; w.rec_stride = a.rec_stride; w.stats = wv.stats;
    WideCopies wc;
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < MAXL; ++l) wc.w[n][l] = l < num_layers ? a.L.w[n][l] : n_params;
    wc.NL = num_layers; wc.Hd = hidden; wc.D = D; wc.wop = wv.wop;
    wc.wop3 = bf3k ? wv.wop3 : nullptr;
    // no K7 operand copies (offsets past the bucket); K7w's if a next slice is named
    w.copies = operand_copies(n_params, nullptr, 1, nullptr, nullptr, tail && tail->next_idx ? &wc : nullptr);
    return launch_mlp_tail(w, tail, s);
}

extern "C" int aurppo_mlp_wide_ppo_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M,
                                            int D, int A, int continuous, int hidden, int num_layers, const float* params,
                                            const int* layout_h, int n_params, float* grads, double clip, double ent_coef,
                                            double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace,
                                            void* stream, void* ev_begin, void* ev_end) {
    return wide_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, num_layers, params, layout_h, n_params, grads, clip,
                          ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, ev_begin, ev_end, nullptr,
                          "aurppo_mlp_wide_ppo_step_f32");
}

extern "C" int aurppo_mlp_wide_ppo_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx,
                                                 int M, int D, int A, int continuous, int hidden, int num_layers, float* params,
                                                 const int* layout_h, int n_params, float* grads, double clip, double ent_coef,
                                                 double vf_coef, int norm_adv, int vloss_mode, float* out_scalars,
                                                 float* exp_avg, float* exp_avg_sq, double max_norm, const float* lr_dev,
                                                 float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                                 const int32_t* next_idx, int next_M, int chained, void* workspace, void* stream) {
    AURPPO_REQUIRE(exp_avg && exp_avg_sq && lr_dev && step_dev && out_norm, AURPPO_EINVAL,
                   "aurppo_mlp_wide_ppo_minibatch_f32: null optimizer pointer");
    AURPPO_REQUIRE(!next_idx || next_M > 0, AURPPO_ESHAPE, "aurppo_mlp_wide_ppo_minibatch_f32: next_M=%d", next_M);
    MlpTail t;
    t.params_rw = params; t.exp_avg = exp_avg; t.exp_avg_sq = exp_avg_sq; t.max_norm = max_norm; t.lr_dev = lr_dev;
    t.step_dev = step_dev; t.beta1 = beta1; t.beta2 = beta2; t.eps = eps; t.out_norm = out_norm;
    t.next_idx = next_idx; t.next_M = next_idx ? next_M : 0; t.chained = chained ? 1 : 0; t.grad_only = 0;
    return wide_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, num_layers, params, layout_h, n_params, grads, clip,
                          ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, nullptr, nullptr, &t,
                          "aurppo_mlp_wide_ppo_minibatch_f32");
}

extern "C" int aurppo_mlp_wide_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                       int num_layers, const float* params, const int* layout_h, int n_params, float* actions,
                                       float* logp, float* value, void* workspace, void* stream) {
    const char* who = "aurppo_mlp_wide_act_f32";
    AURPPO_REQUIRE(obs && params && layout_h && value && workspace, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(!noise || (actions && logp), AURPPO_EINVAL, "%s: sampling needs actions and logp outputs", who);
    int rc = check_shape(D, A, continuous, hidden, num_layers, who);
    if (rc != AURPPO_OK) return rc;
    AURPPO_REQUIRE(N > 0 && n_params > 0, AURPPO_ESHAPE, "%s: N=%d n_params=%d", who, N, n_params);
    AURPPO_REQUIRE(aligned_to(workspace, 64), AURPPO_EINVAL, "%s: workspace not 64-byte aligned", who);
    WideArgs a;
    rc = wide_args(a, obs, params, D, A, continuous, hidden, num_layers, layout_h, n_params, who);
    if (rc != AURPPO_OK) return rc;
    a.noise = noise; a.out_actions = actions; a.out_logp = logp; a.out_value = value;
    a.N = N;
    a.net_base = noise ? 0 : 1;
    a.net_count = noise ? 2 : 1;
    const WideWs wv = wide_ws(workspace, 0, 0);      // the operand copies sit in front of the slabs
    a.wop = wv.wop;
    hipStream_t s = (hipStream_t)stream;
    rc = wide_prep(false, a, num_layers, 0, 0, wv, s);
    if (rc != AURPPO_OK) return rc;
    const int grid = ((N + R - 1) / R) * a.net_count;
    return wide_with_nl(num_layers, [&](auto n) {
        constexpr int NL = decltype(n)::value;
        return wide_launch<k_mlpw_act<NL>>("k_mlpw_act", grid, wide_lds_bytes<false, NL>(1), s, a);
    });
}
