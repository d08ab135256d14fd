// Shared pieces of the fused MLP kernels (K7 k_mlp_step2 / k_mlp_step3, K8 k_mlp_act, K7w / K8w): tile constants, the
// argument block, the fp32 MFMA micro-kernels and the tanh used by every variant; the workspace carver; what K7's and K7w's
// host paths do alike in front of their step kernel; the advantage partial sums; every operand-copy layout's index function.
#pragma once
#include "ppo_math.h"

// Diagnostic build knob: s_setprio around the MFMA chunks of mma32 (0 = off).
#ifndef AURPPO_MMA_PRIO
#define AURPPO_MMA_PRIO 0
#endif

namespace aurppo_mlp {

constexpr int H = 64;        // hidden width
constexpr int R = 32;        // rows per tile
constexpr int LD = H + 1;    // LDS row stride of every 64-wide matrix (odd: conflict-free both ways)
constexpr int AP = 16;       // padded head width (action_dim <= 16)
constexpr int LDO = AP + 1;
constexpr int kThreads = 256;
constexpr int kMaxGrid = 256;
constexpr int kStatBlocks = 256;

// K7's gradient slabs: (kMaxGrid, slab_stride) floats, slab b's parameter p at b * slab_stride + p (bucket order).  The stride is
// padded to 64 floats so that every slab row starts on a 256-B boundary: k_mlp_reduce_x4 (mlp_tail.hip) then reads a row's 64 parameters of a
// workgroup as 16 aligned 16-byte loads (two whole 128-B lines).  The padding is never written and never read.
__host__ __device__ constexpr int slab_stride(int n_params) { return (n_params + 63) & ~63; }

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MlpLayout {  // float offsets into the flat parameter / gradient bucket
    int w1[2], b1[2], w2[2], b2[2], w3[2], b3[2];  // [0] actor, [1] critic
    int logstd;
    int n_params;
};

struct MlpArgs {
    const float* obs;      // (B, D) rollout observations (flattened buffer)
    const float* actions;  // (B, A)
    const float4* rec;     // (B, 4) {old_logp, adv, ret, old_v}; packed mode: (B, 16) with the action row in floats 4..15
    int rec_stride;        // float4s per record: 1, or 4 in packed mode (actions == nullptr)
    const int32_t* idx;    // (M,) minibatch permutation slice
    const float* params;   // flat bucket
    float* slabs;          // (grid, slab_stride(n_params)) per-workgroup gradient slabs
    double* loss_part;     // (grid, 8)
    unsigned long long* stamps;  // diagnostic build: (grid, 16) cycle counters
    unsigned* tile_counter;  // next tile to hand out ([0]), zeroed by k_adv_stats_idx / k_mlp_reduce
    float* w1op;           // two-set kernel: W1 slices in MFMA B-operand order, [4 waves][32 k-steps][64 lanes]
    const void* wop3;      // k_mlp_step3: bf16 planes of the weights in operand order (bf16x3.h)
    const double* stats;   // (kStatBlocks, 2) advantage partial sums
    int n_stat_blocks;
    int D, A;
    int continuous;        // 1: Gaussian head (A action dims), 0: Categorical head (A logits, one action index)
    int static_tiles;      // diagnostic (AURPPO_STATIC_TILES): set s takes tiles s, s + S, s + 2S, ... -- a fixed summation order
    MlpLayout L;
    PpoHyper h;
};

// accumulator element e of a 32x32 MFMA block: (row, col) owned by this lane
__device__ __forceinline__ int acc_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

// acc += A(32 x K) * B(K x 32); a_at(i,k) / b_at(k,j) fetch operand elements (LDS reads).
// K is a compile-time constant: the chain is fully unrolled in chunks of CH MFMAs whose 2*CH operand
// reads are issued one chunk ahead -- with one wave per SIMD nobody else hides the LDS latency (CH = 8);
// the two-set kernel runs two waves per SIMD and has half the registers, so it uses CH = 4.
template <int K, int CH = 8, bool FENCE = false, class FA, class FB>
__device__ __forceinline__ void mma32(f32x16& acc, FA a_at, FB b_at, int lane) {
    static_assert(K % (2 * CH) == 0, "K must be a multiple of the chunk depth");
    const int ij = lane & 31, kk = lane >> 5;
    float av[2][CH], bv[2][CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        av[0][u] = a_at(ij, 2 * u + kk);
        bv[0][u] = b_at(2 * u + kk, ij);
    }
#pragma unroll
    for (int c = 0; c < K / (2 * CH); ++c) {
        if (c + 1 < K / (2 * CH)) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                av[(c + 1) & 1][u] = a_at(ij, 2 * CH * (c + 1) + 2 * u + kk);
                bv[(c + 1) & 1][u] = b_at(2 * CH * (c + 1) + 2 * u + kk, ij);
            }
        }
#if AURPPO_MMA_PRIO
        __builtin_amdgcn_s_setprio(AURPPO_MMA_PRIO);
#endif
#pragma unroll
        for (int u = 0; u < CH; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c & 1][u], bv[c & 1][u], acc, 0, 0, 0);
#if AURPPO_MMA_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        // FENCE pins the pipeline depth to what is written here: without it the scheduler hoists every operand
        // read of the unrolled chain to the top, which costs ~2K registers the two-set kernel does not have.
        if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
}

template <int K, int CH = 8, class FA, class FB>
__device__ __forceinline__ void mma32(f32x16& acc, FA a_at, FB b_at) {
    mma32<K, CH, false>(acc, a_at, b_at, (int)(threadIdx.x & 63));
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16x16 output tile: acc += A(16 x K) * B(K x 16) on v_mfma_f32_16x16x4_f32 (lane l: A[l&15][l>>4],
// B[l>>4][l&15]; C: col = l&15, row = 4*(l>>4) + reg).  Two interleaved accumulators hide the 40-cycle
// dependent latency behind the 32-cycle issue interval; operands are read one 8-MFMA chunk ahead.
template <int K, bool FENCE = false, class FA, class FB>
__device__ __forceinline__ f32x4 mma16(FA a_at, FB b_at, int lane) {
    static_assert(K % 32 == 0, "K must be a multiple of 32");
    const int ij = lane & 15, kk = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float av[2][8], bv[2][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        av[0][u] = a_at(ij, 4 * u + kk);
        bv[0][u] = b_at(4 * u + kk, ij);
    }
#pragma unroll
    for (int c = 0; c < K / 32; ++c) {
        if (c + 1 < K / 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                av[(c + 1) & 1][u] = a_at(ij, 32 * (c + 1) + 4 * u + kk);
                bv[(c + 1) & 1][u] = b_at(32 * (c + 1) + 4 * u + kk, ij);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c & 1][u], bv[c & 1][u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c & 1][u + 1], bv[c & 1][u + 1], acc1, 0, 0, 0);
        }
        if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
    return acc0 + acc1;
}

template <int K, class FA, class FB>
__device__ __forceinline__ f32x4 mma16(FA a_at, FB b_at) {
    return mma16<K, false>(a_at, b_at, (int)(threadIdx.x & 63));
}

// tanh(x) = 1 - 2 / (e^{2x} + 1): v_exp + v_rcp, absolute error ~1e-7 everywhere (saturates cleanly)
__device__ __forceinline__ float tanh_fast(float x) {
    const float e = __expf(2.0f * x);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// tanh(acc + bias) with the bias folded into the exponent's multiply: e^{2 (acc + bias)} = 2^{acc * c + bias * c}, c = 2 log2(e) -- one
// fused multiply-add in front of v_exp instead of an add and a multiply (bc = bias * kTanhC, formed once per block)
constexpr float kTanhC = 2.8853900817779268f;
__device__ __forceinline__ float tanh_fast_fma(float acc, float bc) {
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc, kTanhC, bc));
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// All-reduce over aligned groups of 8 lanes with DPP moves (no LDS traffic): lane i <- i ^ 7 (row_half_mirror),
// then i ^ 1 and i ^ 2 (quad_perm) -- together every lane has combined all 8.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float sum8(float v) {
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    return v;
}
__device__ __forceinline__ float max8(float v) {
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    return v;
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

// A caller's workspace as regions at multiples of 64 bytes from its start, taken in order, and the size the caller is told to provide:
// the regions' sizes plus the slack each was given for the rounding behind it (>= 64 where the size is no multiple of 64).  A family's
// carve-up is ONE list of take() calls: its pointers and its *_workspace_bytes both come from that list.
struct WsCarver {
    uintptr_t at;        // where the next region starts
    size_t bytes = 0;    // what the *_workspace_bytes entry point reports
    explicit WsCarver(void* workspace) : at(reinterpret_cast<uintptr_t>(workspace)) {}
    template <class T>
    T* take(size_t n_bytes, size_t slack = 0) {
        T* const p = reinterpret_cast<T*>(at);
        at += (n_bytes + 63) / 64 * 64;
        bytes += n_bytes + slack;
        return p;
    }
};

// mlp2.hip: the two-tile-set variant of K7 (8 waves per workgroup); same arguments, same slab / loss_part outputs.
size_t mlp_step2_lds_bytes();
int launch_mlp_step2(const MlpArgs& a, int grid, hipStream_t s);
// mlp3.hip: the same step on bf16 MFMAs over three-way bf16 splits (AURPPO_K7_VARIANT=3); its operand-order weight copies (bf16x3.h:
// wop3_prepare, run by k_adv_stats_idx; refreshed by k_adam_chain, mlp_tail.hip)
size_t mlp_step3_lds_bytes();
size_t mlp_step3_wop_bytes();
int launch_mlp_step3(const MlpArgs& a, int grid, hipStream_t s);
// ---- What K7's step path (mlp.hip: mlp_step_impl) and K7w's (mlp_wide.hip: wide_step_impl) do alike before their main kernel.  The
// tail behind it -- slab reduce, optimizer launch -- is mlp_tail.h.
// The refusals both make, in their order: null pointer, packed records, then the family's own shape checks (`shape_checks`: () -> return
// code), M / n_params, vloss_mode.
template <class ShapeChecks>
int check_step_args(const char* who, bool pointers, const float* actions, int continuous, int A, int M, int n_params, int vloss_mode,
                    ShapeChecks shape_checks) {
    AURPPO_REQUIRE(pointers, AURPPO_EINVAL, "%s: null pointer", who);
    // actions == NULL: packed records -- rec is (B, 16), floats 4.. of a record hold the sample's action row
    AURPPO_REQUIRE(actions || (continuous ? A : 1) <= 12, AURPPO_ESHAPE, "%s: packed records hold at most 12 action floats (action_dim=%d)", who, A);
    if (const int rc = shape_checks()) return rc;
    AURPPO_REQUIRE(M > 0 && n_params > 0, AURPPO_ESHAPE, "%s: M=%d n_params=%d", who, M, n_params);
    AURPPO_REQUIRE(vloss_mode >= 0 && vloss_mode <= 2, AURPPO_EINVAL, "%s: bad vloss_mode %d", who, vloss_mode);
    return AURPPO_OK;
}
// The parameter offsets every MLP entry of the 2 x 64 policy is given (K7, K8, the optimizer launch, K16), read and range-checked.
// layout_h: w1a,b1a,w2a,b2a,w3a,b3a, w1c,b1c,w2c,b2c,w3c,b3c, logstd (read, and checked, only for a Gaussian head)
inline int fill_layout(MlpLayout& L, const int* layout_h, int continuous, int n_params, const char* who) {
    for (int n = 0; n < 2; ++n) {
        L.w1[n] = layout_h[6 * n + 0]; L.b1[n] = layout_h[6 * n + 1]; L.w2[n] = layout_h[6 * n + 2];
        L.b2[n] = layout_h[6 * n + 3]; L.w3[n] = layout_h[6 * n + 4]; L.b3[n] = layout_h[6 * n + 5];
    }
    L.logstd = continuous ? layout_h[12] : 0;
    L.n_params = n_params;
    for (int k = 0; k < (continuous ? 13 : 12); ++k)
        AURPPO_REQUIRE(layout_h[k] >= 0 && layout_h[k] < n_params, AURPPO_ESHAPE, "%s: layout[%d]=%d", who, k, layout_h[k]);
    return AURPPO_OK;
}
// CUs the step kernels leave to the side stream's shuffle kernels: AURPPO_MLP_SPARE_CUS, default 8 (one per XCD)
inline int spare_cus() {
    const int k = aurppo_knobs().k7_spare_cus;
    return k >= 0 ? k : 8;
}
// workgroups that form a minibatch's advantage partial sums: four elements per thread, at most kStatBlocks
inline int stat_blocks_for(int M) {
    const int sb = (M + kThreads * 4 - 1) / (kThreads * 4);
    return sb > kStatBlocks ? kStatBlocks : sb;
}
// One thread's share of a minibatch's advantage partial sums: elements first, first + step, ... in that order (the sums are the
// same bits as the plain loop's), four index loads and then four record loads in flight at a time -- the plain loop paid two
// dependent memory round trips per element.
__device__ __forceinline__ void adv_partial_sums(const float4* __restrict__ rec, int rec_stride, const int32_t* __restrict__ idx,
                                                 int M, int first, int step, double& s, double& q) {
    int i = first;
    for (; i + 3 * step < M; i += 4 * step) {
        const int j0 = idx[i], j1 = idx[i + step], j2 = idx[i + 2 * step], j3 = idx[i + 3 * step];
        const float x0 = rec[(size_t)j0 * rec_stride].y, x1 = rec[(size_t)j1 * rec_stride].y;
        const float x2 = rec[(size_t)j2 * rec_stride].y, x3 = rec[(size_t)j3 * rec_stride].y;
        s += (double)x0; q += (double)x0 * (double)x0;
        s += (double)x1; q += (double)x1 * (double)x1;
        s += (double)x2; q += (double)x2 * (double)x2;
        s += (double)x3; q += (double)x3 * (double)x3;
    }
    for (; i < M; i += step) {
        const double x = (double)rec[(size_t)idx[i] * rec_stride].y;
        s += x;
        q += x * x;
    }
}

// ---- Operand-order copies of the weights.  Each layout has ONE index function, here, with its inverse beside it (tied by the
// static_assert below): the kernel that builds a copy walks its entries and asks the inverse what each holds, the optimizer launch
// that refreshes a copy in place (mlp_tail.hip: refresh_operand_copies) asks the index where a weight sits.
// k_mlp_step2's w1op (built by k_adv_stats_idx): W1 of both nets as the B operand of the layer-1 chain, [4 roles][32 steps][64 lanes]:
// role net * 2 + cb, step m, lane l hold W1[net][cb*32 + (l & 31)][2m + (l >> 5)], zero beyond D -- wave `role` reads its slice with 32
// fully coalesced loads per tile.  (k_mlp_step3's bf16 planes of W1 / W2: bf3::wop3_places / wop3_prepare, bf16x3.h.)
constexpr int kW1opFloats = 4 * 32 * kWave;
__host__ __device__ constexpr int w1op_index(int net, int row, int col) {
    return ((net * 2 + (row >> 5)) * 32 + (col >> 1)) * kWave + (row & 31) + 32 * (col & 1);
}
struct W1opPlace { int net, row, col; };
__host__ __device__ constexpr W1opPlace w1op_place(int e) {     // entry e holds W1[net][row][col]
    return {e >> 12, ((e >> 11) & 1) * 32 + (e & 31), 2 * ((e >> 6) & 31) + ((e >> 5) & 1)};
}

// K7w's fp32 copies of the hidden layers (k_mlpw_prep builds, k_mlpw_step / k_mlpw_act stream): [net][layer][fwd | bwd][4 x 4 blocks]
// [lane][16 steps].  Copy (net, l, dir) is a B operand -- forward (dir 0) B[k][j] = W[j][k], backward (dir 1, layers >= 1) B[k][j] =
// W[k][j] -- and entry (block (jb, kb), lane, m) holds B[kb*32 + 2m + (lane >> 5)][jb*32 + (lane & 31)], zero beyond the layer's widths.
constexpr int MAXL = 3;             // hidden layers of a K7w net
constexpr int kOpBlk = 64 * 16;     // floats of one 32x32 block in operand order: [lane][16 k-steps]
constexpr int kOpLayer = 16 * kOpBlk;                 // 4 x 4 blocks
constexpr int kOpFloats = 2 * MAXL * 2 * kOpLayer;    // [net][layer][fwd | bwd]
__host__ __device__ constexpr size_t op_copy(int net, int l, int dir) { return (size_t)((net * MAXL + l) * 2 + dir) * kOpLayer; }
__host__ __device__ constexpr int op_entry(int jb, int kb, int lane, int m) { return (jb * 4 + kb) * kOpBlk + lane * 16 + m; }
__host__ __device__ constexpr size_t op_at(int net, int l, int dir, int jb, int kb, int lane, int m) { return op_copy(net, l, dir) + op_entry(jb, kb, lane, m); }
__host__ __device__ constexpr size_t op_index(int net, int l, int dir, int row, int col) {   // where W[row][col] sits in copy (net, l, dir)
    const int j = dir == 0 ? row : col, k = dir == 0 ? col : row;
    return op_at(net, l, dir, j >> 5, k >> 5, (j & 31) + 32 * (k & 1), (k & 31) >> 1);
}
// ... and back: the B[k][j] that entry (block (jb, kb), lane, m) holds, for a builder that walks the entries
__host__ __device__ constexpr int op_j(int jb, int lane) { return jb * 32 + (lane & 31); }
__host__ __device__ constexpr int op_k(int kb, int lane, int m) { return kb * 32 + 2 * m + (lane >> 5); }

// K7w's bf16-plane copies (built by k_mlpw3_prep, streamed by k_mlpw3_step): slot (net, layer, direction) x column block of 32 x
// k-step of 16 x plane x lane x 8, the same B operands: entry (cb, ks, p, lane, j) holds plane p of B[16 ks + 8 (lane >> 5) + j][cb*32 +
// (lane & 31)].  A value's three planes lie kOp3Plane apart.
constexpr int kOp3Ks = 8;                          // k-steps of a weight slice (128 / 16)
constexpr int kOp3Plane = 64 * 8;                  // bf16 elements of one plane of one k-step
constexpr int kOp3Slice = kOp3Ks * 3 * kOp3Plane;  // one (slot, column block) slice
constexpr int kOp3Slot = 4 * kOp3Slice;            // one (net, layer, direction)
constexpr int kOp3Elems = 2 * MAXL * 2 * kOp3Slot;
__host__ __device__ constexpr int op3_slot(int net, int l, int dir) { return (net * MAXL + l) * 2 + dir; }
__host__ __device__ constexpr int op3_at(int slot, int cb, int ks, int p, int lane, int j) {
    return slot * kOp3Slot + cb * kOp3Slice + ((ks * 3 + p) * 64 + lane) * 8 + j;
}
__host__ __device__ constexpr int op3_index(int net, int l, int dir, int row, int col) {     // plane 0 of W[row][col] in copy (net, l, dir)
    const int n = dir == 0 ? row : col, k = dir == 0 ? col : row;
    return op3_at(op3_slot(net, l, dir), n >> 5, k >> 4, 0, (n & 31) + 32 * ((k >> 3) & 1), k & 7);
}
// ... and back: the B[k][n] that entry (cb, ks, lane, j) holds, for a builder that walks the entries
__host__ __device__ constexpr int op3_n(int cb, int lane) { return cb * 32 + (lane & 31); }
__host__ __device__ constexpr int op3_k(int ks, int lane, int j) { return 16 * ks + 8 * (lane >> 5) + j; }

constexpr bool operand_places_invert_indices() {      // (every third entry: each field of an entry still takes all its values)
    for (int e = 0; e < kW1opFloats; e += 3) {
        const W1opPlace p = w1op_place(e);
        if (w1op_index(p.net, p.row, p.col) != e) return false;
    }
    for (int e = 0; e < kOpLayer; e += 3) {
        const int m = e & 15, lane = (e >> 4) & 63, kb = (e >> 10) & 3, jb = e >> 12, j = op_j(jb, lane), k = op_k(kb, lane, m);
        if (op_index(1, 2, 0, j, k) != op_at(1, 2, 0, jb, kb, lane, m) || op_index(1, 2, 1, k, j) != op_at(1, 2, 1, jb, kb, lane, m)) return false;
    }
    for (int e = 0; e < 4 * kOp3Ks * 64 * 8; e += 3) {
        const int j = e & 7, lane = (e >> 3) & 63, ks = (e >> 9) & 7, cb = e >> 12, n = op3_n(cb, lane), k = op3_k(ks, lane, j);
        if (op3_index(1, 2, 0, n, k) != op3_at(op3_slot(1, 2, 0), cb, ks, 0, lane, j) || op3_index(1, 2, 1, k, n) != op3_at(op3_slot(1, 2, 1), cb, ks, 0, lane, j)) return false;
    }
    return true;
}
static_assert(operand_places_invert_indices(), "an operand copy's inverse map must undo its index");

// What the optimizer launch needs to refresh K7w's copies: where it drops an updated weight so that the next K7w launch needs no
// prepare pass.  wop == nullptr: nothing to refresh.
struct WideCopies {
    int w[2][MAXL];    // float offsets of the hidden layers' weights in the bucket
    int NL, Hd, D;
    float* wop;
    unsigned short* wop3;   // != nullptr: k_mlpw3_step's bf16-plane copies are the ones to refresh
};

}  // namespace aurppo_mlp
