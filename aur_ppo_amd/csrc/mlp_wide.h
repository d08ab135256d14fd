// What the K7w / K8w sources share: mlp_wide.hip (k_mlpw_prep, k_mlpw_step, k_mlpw_act, the host side and the C entries) and
// mlp_wide3.hip (k_mlpw3_prep, k_mlpw3_step and their launchers).  The argument block and the workspace carve-up, and the passages of
// the two step kernels that are the same text in both: the advantage statistics, the small weights that stay in LDS, the index and
// record prefetch, the tile queue, the head-side column sums and the rows of the slab that do not depend on a build's accumulator
// layout.  Every helper is expanded in place (__forceinline__): an opaque copy or a load inside one stands in the instruction order
// where the call stands.  The __shared__ objects stay declared in the kernels, which hand them in.
// Both includers say `#pragma clang fp contract(fast)` in front of their includes, and this code is written for that mode.
#pragma once
#include <type_traits>

#include "mlp_bf3.h"

namespace aurppo_mlp {

constexpr int HPW = 128;            // widest (padded) layer
constexpr int LDW = HPW + 1;        // LDS row stride of an activation matrix (odd: conflict-free row- and column-wise)
constexpr int kMaxSlabs = 2 * kMaxGrid;               // k_mlp_reduce folds up to 512

struct WideLayout {   // float offsets into the flat parameter / gradient bucket; layer NL is the head
    int w[2][MAXL + 1], b[2][MAXL + 1];
    int logstd, n_params;
};

struct WideArgs {
    const float* obs;      // (B, D)
    const float* actions;  // (B, AW) or nullptr (packed records)
    const float4* rec;     // (B, 4) | (B, 16) packed
    int rec_stride;
    const int32_t* idx;    // (M,)
    const float* params;
    const float* wop;      // operand-order copies (k_mlpw_prep)
    const unsigned short* wop3;   // k_mlpw3_step: bf16 planes of the hidden layers in operand order (k_mlpw3_prep)
    float* slabs;          // (pairs, n_params)
    double* loss_part;     // (pairs, 8)
    const double* stats;   // (n_stat_blocks, 2)
    unsigned* tile_counter;   // [2]: next tile to hand out, per net (one-net workgroups) or [0] alone (both-net workgroups)
    int n_stat_blocks;
    int D, A, Hd, continuous;
    WideLayout L;
    PpoHyper h;
    // rollout step
    const float* noise;
    float* out_actions;
    float* out_logp;
    float* out_value;
    int N, net_base, net_count;
    int static_tiles;      // diagnostic (AURPPO_STATIC_TILES): workgroup p of P takes tiles p, p + P, ... -- a fixed summation order
};

struct WideWs {
    double* stats;       // (kStatBlocks, 2)
    double* loss_part;   // (kMaxSlabs, 8)
    float* wop;          // kOpFloats
    unsigned* tile_counter;   // [2] (+ padding to 64 B)
    float* slabs;        // (kMaxSlabs, n_params)
    double* sq_part;     // (ceil(n_params / 64)) clip partial sums left by k_mlp_reduce
    unsigned short* wop3;   // k_mlpw3_step's bf16-plane operand copies (kOp3Elems), behind everything else
    size_t bytes;           // aurppo_mlp_wide_workspace_bytes
};
inline WideWs wide_ws(void* workspace, int n_params, int slab_cap) {
    WsCarver c(workspace);
    WideWs v;
    v.stats = c.take<double>(sizeof(double) * 2 * kStatBlocks);
    v.loss_part = c.take<double>(sizeof(double) * 8 * kMaxSlabs);
    v.wop = c.take<float>(sizeof(float) * kOpFloats);
    v.tile_counter = c.take<unsigned>(sizeof(unsigned) * 16);
    v.slabs = c.take<float>(sizeof(float) * (size_t)slab_cap * (size_t)n_params, 64);
    v.sq_part = c.take<double>(sizeof(double) * (size_t)((n_params + 63) / 64), 128);
    v.wop3 = c.take<unsigned short>(sizeof(unsigned short) * (size_t)kOp3Elems, 64);
    v.bytes = c.bytes;
    return v;
}

// K7w / K8w launches ask for the LDS they raise the kernel's limit to
template <auto Kernel>
int wide_launch(const char* name, int grid, size_t lds, hipStream_t s, const WideArgs& a) {
    return launch_dyn_lds<Kernel>(name, grid, kThreads, lds, lds, s, a);
}
// A run-time layer count as a template argument, named once:  wide_with_nl(nl, [&](auto n) { launch k<decltype(n)::value, ...> })
template <class F>
int wide_with_nl(int num_layers, F&& f) {
    if (num_layers == 1) return f(std::integral_constant<int, 1>{});
    if (num_layers == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

// mlp_wide3.hip: the step on bf16 MFMAs over three-way bf16 splits (the default beyond 64 units; AURPPO_K7W_VARIANT=2 keeps
// k_mlpw_step) and the prepare pass that leaves its operand copies in wop3 -- same arguments, slabs and loss partials as k_mlpw_step
int launch_mlpw3_prep(const WideArgs& a, int num_layers, int M, int sb, double* stats, unsigned* tile_counter, unsigned short* wop3, hipStream_t s);
int launch_mlpw3_step(const WideArgs& a, int num_layers, int grid, hipStream_t s);

// ---- prepare kernels: the counter reset, and the first n_stat_blocks workgroups' partial (sum, sum of squares) of the minibatch's
// advantages.  true: this workgroup was one of those and is done.
__device__ __forceinline__ bool prep_stats(double (&sc)[2][4], const float4* __restrict__ rec, int rec_stride,
                                           const int32_t* __restrict__ idx, int M, double (*__restrict__ stats)[2], int n_stat_blocks,
                                           unsigned* __restrict__ tile_counter) {
    if (tile_counter && blockIdx.x == 0 && threadIdx.x < 2) tile_counter[threadIdx.x] = 0u;
    if ((int)blockIdx.x >= n_stat_blocks) return false;
    double s = 0.0, q = 0.0;
    adv_partial_sums(rec, rec_stride, idx, M, blockIdx.x * 256 + threadIdx.x, n_stat_blocks * 256, s, q);
    const double bs = block_sum<4>(s, sc[0]);
    const double bq = block_sum<4>(q, sc[1]);
    if (threadIdx.x == 0) {
        stats[blockIdx.x][0] = bs;
        stats[blockIdx.x][1] = bq;
    }
    return true;
}

// ---- step kernels, ahead of the tile loop
// hidden biases (HP_ slots per layer, zero beyond Hd), head bias, log-std and sIvar = 1 / sigma^2 (step) | sigma (act_mode)
template <int NL, int HP_>
__device__ __forceinline__ void stage_biases(const WideArgs& a, int net, float* sB, float* sB3, float* sLs, float* sIvar, bool act_mode) {
    const int tid = threadIdx.x, Hd = a.Hd, out_dim = net == 0 ? a.A : 1;
    for (int e = tid; e < NL * HP_; e += kThreads) {
        const int l = e / HP_, c = e - l * HP_;
        sB[e] = c < Hd ? a.params[a.L.b[net][l] + c] : 0.0f;
    }
    if (tid < AP) {
        sB3[tid] = tid < out_dim ? a.params[a.L.b[net][NL] + tid] : 0.0f;
        const float ls = (a.continuous && tid < a.A) ? a.params[a.L.logstd + tid] : 0.0f;
        const float sd = expf(ls);
        sLs[tid] = ls;
        sIvar[tid] = act_mode ? sd : 1.0f / (sd * sd);
    }
}
// the prepare pass's stat blocks folded to the minibatch's advantage mean / std (thread 0 writes them; the caller's barrier follows)
__device__ __forceinline__ void fold_adv_stats(const WideArgs& a, double (&s_red)[2][kThreads / kWave], float& s_mean, float& s_std) {
    const int tid = threadIdx.x;
    double sm = 0.0, q = 0.0;
    for (int b = tid; b < a.n_stat_blocks; b += kThreads) {
        sm += a.stats[2 * b];
        q += a.stats[2 * b + 1];
    }
    const double ts = block_sum<kThreads / kWave>(sm, s_red[0]);
    const double tq = block_sum<kThreads / kWave>(q, s_red[1]);
    if (tid == 0) {
        adv_mean_std(ts, tq, a.h.M, s_mean, s_std);
    }
}

// ---- prefetch.  Every load is unconditional (a piece that is not real reads element 0) and nothing is computed from its result
// where it is asked for: a conditional load is a write to its destination on the other path, and the wait the compiler puts in
// front of that write -- or in front of an `ok ? v : 0` select -- is a wait for every load above it.
// thread tid's entry of a tile's index row, -1 beyond the minibatch
__device__ __forceinline__ int load_idx(const WideArgs& a, int n_tiles, int tile) {
    const int m = tile * R + (int)threadIdx.x;
    return (tile < n_tiles && m < a.h.M) ? a.idx[m] : -1;
}
// the index row of a tile further ahead: raw value + whether it is real
__device__ __forceinline__ void prefetch_idx(const WideArgs& a, int n_tiles, int tile, bool& n_ok, int& n_raw) {
    int tq = threadIdx.x;
    asm volatile("" : "+v"(tq));
    const int m = tile * R + (tq & (R - 1));
    n_ok = tile < n_tiles && m < a.h.M;
    n_raw = a.idx[n_ok ? m : 0];
}
// where the action rows are: beside the records, or in floats 4..15 of a packed record
struct ActRows {
    const float* base;
    int stride;
};
__device__ __forceinline__ ActRows act_rows(const WideArgs& a, int AW) {
    return {a.actions ? a.actions : reinterpret_cast<const float*>(a.rec) + 4, a.actions ? AW : 16};
}
// a thread's two pieces of the tile's action rows: load(u, address) asks for piece u; bit 16 + u of xok says whether it is real
template <class Load>
__device__ __forceinline__ void prefetch_actions(const int* sidx, int tq, const ActRows& ar, int AW, unsigned& xok, Load load) {
    int sa[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) sa[u] = sidx[(tq + u * kThreads) >> 4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = tq & 15;
        const bool ok = sa[u] >= 0 && c < AW;
        const unsigned row = ok ? (unsigned)sa[u] : 0u, col = ok ? (unsigned)c : 0u;
        load(u, ar.base + ((size_t)row * (unsigned)ar.stride + col));
        xok |= ok ? (1u << (16 + u)) : 0u;
    }
}
// ... and the record of row tq & (R - 1) (every thread, no branch)
__device__ __forceinline__ void prefetch_record(const WideArgs& a, const int* sidx, int tq, int& p_src, float4& p_rec) {
    p_src = sidx[tq & (R - 1)];
    p_rec = a.rec[(size_t)(p_src >= 0 ? p_src : 0) * a.rec_stride];
}

// ---- the tile queue.  Tiles are handed out by a counter, not strided statically: a workgroup that starts late (its CU held by one
// of the side stream's shuffle kernels) then simply takes fewer -- with static striding every launch that overlapped them ran at the
// pace of its latest workgroup (in-situ 247 us min, 443 max).  s_tile[(it + k) & 3], k = 0..3: the tiles this workgroup works on
// next; rows are fetched one tile ahead, indices two to three.
struct TileQueue {
    unsigned* ctr;     // this net's counter
    bool stat;         // AURPPO_STATIC_TILES: workgroup `first` of n_wg takes tiles first, first + n_wg, ...
    int first, n_wg;   // n_wg: workgroups that share this net's tiles
};
// (thread 0) four consecutive tiles to start with; later ones one at a time (ids only ever grow)
__device__ __forceinline__ void tile_queue_start(const TileQueue& q, int (&s_tile)[4]) {
    if (q.stat) {
        s_tile[0] = q.first; s_tile[1] = q.first + q.n_wg; s_tile[2] = q.first + 2 * q.n_wg; s_tile[3] = q.first + 3 * q.n_wg;
    } else {
        const int t0 = (int)atomicAdd(q.ctr, 4u);
        s_tile[0] = t0; s_tile[1] = t0 + 1; s_tile[2] = t0 + 2; s_tile[3] = t0 + 3;
    }
}
// (thread 0) the tile after the three already known, while the workgroup is on `tile`
__device__ __forceinline__ int tile_queue_next(const TileQueue& q, int tile) {
    return q.stat ? tile + 4 * q.n_wg : (int)atomicAdd(q.ctr, 1u);
}

// ---- head side: lane < AP sums column `lane` of the head gradients (d b3), lane - AP < AP that of the d logstd terms
__device__ __forceinline__ float head_colsum(const float* sOut, const float* sDls, int lane) {
    const float* src = lane < AP ? sOut + lane : sDls + (lane - AP);
    float cs = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) cs += src[r * LDO];
    return cs;
}

// ---- the slab: the rows that do not depend on a build's accumulator layout.  The head-side column sums of head_colsum's wave ...
template <int NL>
__device__ __forceinline__ void slab_head_sums(float* slab, const WideArgs& a, int lane, float g_head) {
    if (lane < a.A) slab[a.L.b[0][NL] + lane] = g_head;
    if (a.continuous && lane >= AP && lane - AP < a.A) slab[a.L.logstd + lane - AP] = g_head;
}
// ... and (one thread per workgroup) this net's loss sums v = {pg, ent, okl, kl, cf | vl}; the critic also leaves its head bias gradient
template <int NL>
__device__ __forceinline__ void loss_record(const WideArgs& a, float* slab, int pair, int net, const double* v, float g_b3c, float mean,
                                            float std) {
    double* lp = a.loss_part + (size_t)pair * 8;   // {pg, vl, ent, okl, kl, cf, mean, std}
    if (net == 0) {
        lp[0] = v[0]; lp[2] = v[1]; lp[3] = v[2]; lp[4] = v[3]; lp[5] = v[4];
    } else {
        slab[a.L.b[1][NL]] = g_b3c;
        lp[1] = v[0];
        lp[6] = (double)mean;
        lp[7] = (double)std;
    }
}

}  // namespace aurppo_mlp
