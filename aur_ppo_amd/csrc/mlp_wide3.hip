// k_mlpw3_prep / k_mlpw3_step -- K7w on the bf16 matrix pipe, the default step of the MLP actor-critics wider than 64 (mlp_wide.hip has
// the fp32-MFMA builds, the rollout kernel, the host side and the C entries; mlp_wide.h what the two sources share):
// k_mlpw_step<NL, false>'s geometry (one net per workgroup, four waves, wave w = the w-th 32-column block of every layer, weight
// gradients persistent in registers) with k_mlp_step3's
// arithmetic and operand handling (bf16x3.h: every fp32 operand as three bf16 planes, six v_mfma_f32_32x32x16_bf16 per
// K = 16, fp32 accumulate -- fp32-equivalent, tools/bf16x3_check.hip):
//   * activations are LDS images of bf16 planes -- X as two 64-column X images side by side, H_l (later dZ_l, in place) as
//     128-feature F images -- written straight from the accumulators by the tanh / dZ epilogues; a fragment is one
//     ds_read_b128 or two ds_read_b64_tr_b16 where the fp32 kernel issued a ds_read_b32 per matrix instruction (rocprofv3:
//     k_mlpw_step<3,false> kept the matrix pipe busy 48 % of its 862 us -- on fp32 instructions that cost 2.7x the cycles);
//   * the weights stream from L2 as bf16 planes in B-operand order (k_mlpw3_prep; refreshed in place by the optimizer launch
//     of a chained minibatch), a layer's whole slice (<= 8 k-steps x 3 planes = 96 registers) one phase ahead of its use --
//     one wave per SIMD has the 512-register budget for it next to the 12 x 16 accumulator registers;
//   * head, loss lanes, column sums and the tile queue are k_mlpw_step's; the head gradients also go out as a bf16-plane
//     image ([a 16][s 32]) for the two products that consume them.
// Same arguments, slabs and loss partials as k_mlpw_step: k_mlp_reduce and the optimizer launch do not know the difference.
#pragma clang fp contract(fast)
#include "mlp_wide.h"

using namespace aurppo_mlp;

namespace {

namespace w3 {
using namespace bf3;
constexpr int kFPlaneW = HPW * kFRow;            // F image of 128 features: bytes per plane
constexpr int kXHalf = 3 * kXPlane;              // one 64-column X image (three planes)
constexpr int kW3RowW = 2 * HPW, kW3PlaneW = AP * kW3RowW;       // W3 image [a 16][i 128]
constexpr int kDoRowW = 64, kDoPlaneW = AP * kDoRowW;            // dOut image [a 16][s 32]

// byte offsets of the workgroup's LDS
constexpr int oX = 0;                                  // [2 halves][3 planes][4 KB]
constexpr int oH = oX + 2 * kXHalf;                    // [MAXL][3 planes][8 KB]
constexpr int oW3 = oH + MAXL * 3 * kFPlaneW;          // [3 planes][4 KB]
constexpr int oDo = oW3 + 3 * kW3PlaneW;               // [3 planes][1 KB]
constexpr int oOut = oDo + 3 * kDoPlaneW;              // float [R][LDO]
constexpr int oAct = oOut + 4 * R * LDO;               // float [R][LDO]
constexpr int oDls = oAct + 4 * R * LDO;               // float [R][LDO]
constexpr int oB = oDls + 4 * R * LDO;                 // float [MAXL][HPW]
constexpr int oB3 = oB + 4 * MAXL * HPW;               // float [AP]
constexpr int oLs = oB3 + 4 * AP;                      // float [AP]
constexpr int oIvar = oLs + 4 * AP;                    // float [AP]
constexpr int oRec = oIvar + 4 * AP;                   // float4 [R]
constexpr int oSrc = oRec + 16 * R;                    // int [R]
constexpr int oIdx = oSrc + 4 * R;                     // int [2][R]
constexpr int oStage = (oIdx + 4 * 2 * R + 15) / 16 * 16;      // float [R][HPW]: the next tile's rows as they arrive (LDS-DMA)
constexpr int oStageA = oStage + 4 * R * HPW;          // float [R][16]: its action rows
constexpr int kBytes = oStageA + 4 * R * 16;
static_assert(oH % 16 == 0 && oW3 % 16 == 0 && oDo % 16 == 0 && oOut % 16 == 0 && oRec % 16 == 0, "16-byte alignment of the images");
static_assert(kBytes <= 160 * 1024, "one workgroup per CU");

// LDS-DMA: 16 / 4 bytes per lane from global memory straight into LDS at dst + lane * 16 / 4 (wave-uniform dst), no registers
__device__ __forceinline__ void dma16(const void* src, void* dst_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst_wave_uniform, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const void* src, void* dst_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst_wave_uniform, 4, 0, 0);
}
// sum / maximum over the 16 lanes of a DPP row (every lane gets the result)
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m, 16);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 16));
    return v;
}
// does trip x of a matrix chain run: x < K where the build has a compile-time count (K > 0), else x < the run-time count n
template <int K>
__device__ __forceinline__ bool live(int n, int x) { return K > 0 ? x < K : x < n; }
}  // namespace w3

// wop3 = the bf16 planes of every hidden layer of both nets in operand order (mlp_common.h: op3_at / op3_index), written destination-first so
// that the padding (rows >= Hd, columns >= the layer's input width) is zero without a clearing pass.  The first n_stat_blocks
// workgroups form the advantage partial sums instead (as k_mlpw_prep).
__global__ __launch_bounds__(256) void k_mlpw3_prep(const float* __restrict__ params, WideLayout L, int NL, int D, int Hd,
                                                    unsigned short* __restrict__ wop3, const float4* __restrict__ rec, int rec_stride,
                                                    const int32_t* __restrict__ idx, int M, double (*__restrict__ stats)[2],
                                                    int n_stat_blocks, unsigned* __restrict__ tile_counter) {
    __shared__ double sc[2][4];
    if (prep_stats(sc, rec, rec_stride, idx, M, stats, n_stat_blocks, tile_counter)) return;
    const int b = blockIdx.x - n_stat_blocks, nb = gridDim.x - n_stat_blocks;
    for (int e = b * 256 + threadIdx.x; e < kOp3Elems / 3; e += nb * 256) {      // every (slot, cb, ks, lane, j)
        const int j = e & 7, lane = (e >> 3) & 63, ks = (e >> 9) & 7, cb = (e >> 12) & 3, slot = e >> 14;
        const int dir = slot & 1, nl = slot >> 1, n = nl / MAXL, l = nl - n * MAXL;
        if (l >= NL || (dir == 1 && l == 0)) continue;
        const int in_dim = l == 0 ? D : Hd;
        const float* W = params + L.w[n][l];
        const int k = op3_k(ks, lane, j), c = op3_n(cb, lane);
        // forward: B[k][n = out c] = W[c][k]; backward: B[k = out][n = in c] = W[k][c]
        const int row = dir == 0 ? c : k, col = dir == 0 ? k : c;
        const float v = (row < Hd && col < in_dim) ? W[row * in_dim + col] : 0.0f;
        unsigned p0, p1, p2;
        bf3::split3(v, 0.0f, p0, p1, p2);
        const int at = op3_at(slot, cb, ks, 0, lane, j);
        wop3[at] = (unsigned short)p0;
        wop3[at + kOp3Plane] = (unsigned short)p1;
        wop3[at + 2 * kOp3Plane] = (unsigned short)p2;
    }
}

// Diagnostic build only (-DK7W_STAMPS, tools/k7w_stamps.py): thread 0 of every workgroup accumulates, per segment of the tile loop,
// the cycles up to its closing barrier (work) and inside it (wait)
#ifdef K7W_STAMPS
__device__ unsigned long long g_k7w_stamps[kMaxSlabs][32];
#define WBAR(k)                                                        \
    do {                                                               \
        if (tid == 0) {                                                \
            const unsigned long long t_ = __builtin_readcyclecounter(); \
            wst[(k)] += t_ - wt0;                                      \
            wt0 = t_;                                                  \
        }                                                              \
        __syncthreads();                                               \
        if (tid == 0) {                                                \
            const unsigned long long t_ = __builtin_readcyclecounter(); \
            wst[10 + (k)] += t_ - wt0;                                 \
            wt0 = t_;                                                  \
        }                                                              \
    } while (0)
// (inside a segment: cycles since the last stamp go to slot k, and stay part of the segment's work)
#define WSUB(k)                                                        \
    do {                                                               \
        if (tid == 0) {                                                \
            const unsigned long long t_ = __builtin_readcyclecounter(); \
            wst[(k)] += t_ - wsub0;                                    \
            wsub0 = t_;                                                \
        }                                                              \
    } while (0)
#define WSUB0() do { if (tid == 0) wsub0 = __builtin_readcyclecounter(); } while (0)
#else
#define WBAR(k) __syncthreads()
#define WSUB(k) do { } while (0)
#define WSUB0() do { } while (0)
#endif

// HK > 0: the hidden layers run HK k-steps of 16 (8: 113..128 units, 6: 81..96; zero-padded) and DK > 0: layer 1 runs DK k-steps
// (state width <= 16 DK, zero-padded) -- every trip count of the matrix chains is then a compile-time constant (the phase-level `cb < HB` stays a run-time
// test even so: as a constant it let the compiler's code motion loose across the phases and cost the three-layer build 51 spilled
// registers, among them freshly loaded weight slices).  With run-time counts each k-step sat in
// its own branch, and the wait the compiler places at such a join is lgkmcnt(0): the fragments requested for the NEXT k-step were
// waited for before the current one's products were issued (75-87 cycles per matrix instruction, tools/k7w_stamps.py).
template <int NL, int HK, int DK>
__global__ __launch_bounds__(256, 1) void k_mlpw3_step(const WideArgs a) {
    using namespace w3;
#ifdef K7W_STAMPS
    unsigned long long wst[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) wst[k] = 0;
    unsigned long long wt0 = 0, wsub0 = 0;
    const unsigned long long wt_entry = __builtin_readcyclecounter();
#endif
    extern __shared__ __attribute__((aligned(16))) char ldsb[];
    __shared__ double s_red[2][kThreads / kWave];
    __shared__ float s_mean, s_std;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int net = (int)(blockIdx.x & 1), cb = w, pair = (int)(blockIdx.x >> 1);
    const int D = a.D, A = a.A, Hd = a.Hd;
    const int HB = (Hd + 31) >> 5, DB = (D + 31) >> 5;
    constexpr bool FULL = HK > 0;
    constexpr int HBK = (HK + 1) / 2;         // column blocks of 32 (compile-time builds)
    const int nksD = DK > 0 ? DK : (D + 15) >> 4, nksH = FULL ? HK : (Hd + 15) >> 4, nks2H = FULL ? HBK : (Hd + 31) >> 5;
    const int AW = a.continuous ? A : 1;
    const int out_dim = net == 0 ? A : 1;

    char* const sX = ldsb + oX;
    char* const sW3 = ldsb + oW3;
    char* const sDo = ldsb + oDo;
    float* const sOut = reinterpret_cast<float*>(ldsb + oOut);
    float* const sAct = reinterpret_cast<float*>(ldsb + oAct);
    float* const sDls = reinterpret_cast<float*>(ldsb + oDls);
    float* const sB = reinterpret_cast<float*>(ldsb + oB);
    float* const sB3 = reinterpret_cast<float*>(ldsb + oB3);
    float* const sLs = reinterpret_cast<float*>(ldsb + oLs);
    float* const sIvar = reinterpret_cast<float*>(ldsb + oIvar);
    float4* const sRec = reinterpret_cast<float4*>(ldsb + oRec);
    int* const sSrc = reinterpret_cast<int*>(ldsb + oSrc);
    int* const sIdx = reinterpret_cast<int*>(ldsb + oIdx);
    auto sH = [&](int l) -> char* { return ldsb + oH + l * 3 * kFPlaneW; };

    // ---- what stays in LDS for the whole launch: zeroed images, W3 image, biases, log-std
    {
        u32x4* z = reinterpret_cast<u32x4*>(ldsb);
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int e = tid; e < oOut / 16; e += kThreads) z[e] = zero;          // X, H, W3 and dOut images
        for (int e = tid; e < R * LDO; e += kThreads) sDls[e] = 0.0f;
    }
    __syncthreads();
    for (int e = tid; e < AP * HPW; e += kThreads) {
        const int o = e / HPW, i = e - o * HPW;
        if (o < out_dim && i < Hd) store_plain1(sW3, kW3RowW, kW3PlaneW, o, i, a.params[a.L.w[net][NL] + o * Hd + i]);
    }
    stage_biases<NL, HPW>(a, net, sB, sB3, sLs, sIvar, false);
    fold_adv_stats(a, s_red, s_mean, s_std);
    __syncthreads();
    const float mean = s_mean, denom = s_std + 1e-8f;
    const float invM = 1.0f / (float)a.h.M;
    const float g_ent = -a.h.ent_coef * invM;
    // loss lanes: lane k16 of a DPP row works on head output k16 of rows lrow and lrow + 16
    const int k16 = tid & 15, lrow = tid >> 4;
    const float my_ls = sLs[k16], my_ivar = sIvar[k16];
    float ent_c = 0.0f;                                     // the Gaussian's entropy: the same for every row
    for (int k = 0; k < A; ++k) ent_c += gauss_ent(sLs[k]);

    // persistent accumulators: dW_l blocks (out-block ob, in-block cb), the head's two 16x16 blocks, bias columns
    f32x16 gW[NL][4];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) gW[l][ob] = zero16();
    f32x4 gW3[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float gb[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) gb[l] = 0.0f;
    double l_a = 0, l_b = 0, l_c = 0, l_d = 0, l_e = 0;
    float g_b3c = 0.0f, g_head = 0.0f;

    // ---- this wave's weight slices: a layer's slice (<= 8 k-steps x 3 planes of 16 B per lane) one phase ahead of its use
    // (a wave-uniform base in scalar registers + the lane's 32-bit byte offset + an immediate per fragment; written as 64-bit
    // vector addresses they are formed once, hoisted out of the tile loop and spilled -- every load then waits behind a scratch
    // reload: k_mlp_step3's lesson)
    const char* const wbase0 = reinterpret_cast<const char*>(a.wop3) + 2 * (size_t)(cb * kOp3Slice);
    const char* wbase = wbase0;
    int lane16 = lane * 16;
    // (in two halves: k-steps 0..3 are requested one phase ahead and stay live across the epilogue and the barrier in between;
    // k-steps 4..7 are requested at the top of the phase that uses them, behind the first half's 24 matrix instructions -- held
    // whole, the 96 registers of a slice pushed the kernel's vector registers into scratch)
    bf16x8 wreg[3 * kOp3Ks];
#ifdef K7W_EXP_NO_WLOAD
    int n_loaded = 0, n_loaded_hi = 0;
#endif
    auto load_w = [&](int l, int dir, int nks) {          // first half
#ifdef K7W_EXP_NO_WLOAD       // timing experiment (WRONG results): the weight slices are fetched once per launch
        if (wbase != wbase0 + 0 || n_loaded++) return;
#endif
        int wz = 0;
        asm volatile("" : "+s"(wz));          // (an opaque zero per request: the loads stay where they are asked for)
        const char* m = wbase + wz + 2 * (size_t)(op3_slot(net, l, dir) * kOp3Slot);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            if (ks < nks) {
#pragma unroll
                for (int p = 0; p < 3; ++p) wreg[3 * ks + p] = *reinterpret_cast<const bf16x8*>(m + (ks * 3 + p) * (2 * kOp3Plane) + lane16);
            }
    };
    auto load_w_hi = [&](int l, int dir, int nks) {       // second half
#ifdef K7W_EXP_NO_WLOAD
        if (n_loaded_hi++) return;
#endif
        int wz = 0;
        asm volatile("" : "+s"(wz));
        const char* m = wbase + wz + 2 * (size_t)(op3_slot(net, l, dir) * kOp3Slot);
#pragma unroll
        for (int ks = 4; ks < kOp3Ks; ++ks)
            if (ks < nks) {
#pragma unroll
                for (int p = 0; p < 3; ++p) wreg[3 * ks + p] = *reinterpret_cast<const bf16x8*>(m + (ks * 3 + p) * (2 * kOp3Plane) + lane16);
            }
    };
    auto wfrag = [&](int ks) {
        Frag3 f;
        f.p[0] = wreg[3 * ks + 0];
        f.p[1] = wreg[3 * ks + 1];
        f.p[2] = wreg[3 * ks + 2];
        return f;
    };

    const int n_tiles = (a.h.M + R - 1) / R;
    // staging: 32 chunk slots of 4 columns per row (128 state floats), four slots per thread
    const bool vec4 = (D % 4 == 0) && ((reinterpret_cast<size_t>(a.obs) & 15) == 0);
    unsigned xok = 0u;                // which staged pieces are real (bit u: state piece u of this thread; bit 16 + u: action piece u)
    float4 p_rec = make_float4(0.f, 0.f, 0.f, 0.f);
    int p_src = -1;
    const ActRows arows = act_rows(a, AW);
    char* const sStage = ldsb + oStage;
    char* const sStageA = ldsb + oStageA;
    // The next tile's rows go from HBM straight into an LDS staging area (LDS-DMA: lane l of a wave writes 16 / 4 bytes at the
    // wave's base + l x 16 / 4, which IS the [row][column] order of the pieces a wave asks for), unconditionally (a piece that is
    // not real reads element 0; `xok` remembers which are).  As loads into registers -- sixteen values per thread held for a whole
    // tile in a kernel that has no register to spare -- their destinations doubled as temporaries, and the waits the compiler put
    // in front of those reuses stood the wave through the gathers' HBM latency in the middle of layer 1 (tools/k7w_stamps.py: F1 took
    // 7.5-8.1 k cycles for its 24 matrix instructions).
    auto prefetch = [&](const int* sidx) {
        int tq = tid;
        asm volatile("" : "+v"(tq));       // (an opaque copy: what is derived from it is formed here each time, not once and spilled)
        // (the rows' indices are read from LDS first, all of them, and a piece that is not real is pointed at element 0 by 32-bit
        // selects: written as `ok ? row * D + c : 0` the 64-bit product sat in a branch per piece, each behind its own LDS wait --
        // 1.8 k cycles to issue eight requests, tools/k7w_stamps.py)
        xok = 0u;
        if (vec4) {
            int src[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) src[u] = sidx[(tq + u * kThreads) >> 5];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c4 = (tq & 31) * 4;
                const bool ok = src[u] >= 0 && c4 < D;
                const unsigned row = ok ? (unsigned)src[u] : 0u, col = ok ? (unsigned)c4 : 0u;
                dma16(a.obs + ((size_t)row * (unsigned)D + col), sStage + (w * 64 + u * kThreads) * 16);
                xok |= ok ? (1u << u) : 0u;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tq + u * kThreads, r = e >> 7, c = e & 127;
                const int s1 = sidx[r];
                const bool ok = s1 >= 0 && c < D;
                const unsigned row = ok ? (unsigned)s1 : 0u, col = ok ? (unsigned)c : 0u;
                dma4(a.obs + ((size_t)row * (unsigned)D + col), sStage + (w * 64 + u * kThreads) * 4);
                xok |= ok ? (1u << u) : 0u;
            }
        }
        if (net == 0)
            prefetch_actions(sidx, tq, arows, AW, xok, [&](int u, const float* p) { dma4(p, sStageA + (w * 64 + u * kThreads) * 4); });
        prefetch_record(a, sidx, tq, p_src, p_rec);
    };
    int n_raw = 0;                    // the index row of the tile three ahead (prefetch_idx)
    bool n_ok = false;
    __shared__ int s_tile[4];
    const TileQueue queue = {a.tile_counter + net, a.static_tiles != 0, pair, (int)(gridDim.x >> 1)};
    if (tid == 0) tile_queue_start(queue, s_tile);
    if (cb < HB) load_w(0, 0, nksD);                        // layer 1's slice for the first tile
    __syncthreads();
    if (tid < R) {
        sIdx[tid] = load_idx(a, n_tiles, s_tile[0]);
        sIdx[R + tid] = load_idx(a, n_tiles, s_tile[1]);
    }
    __syncthreads();
    prefetch(sIdx);
    prefetch_idx(a, n_tiles, s_tile[2], n_ok, n_raw);

#ifdef K7W_STAMPS
    wt0 = __builtin_readcyclecounter();
    wst[20] = wt0 - wt_entry;            // prologue
#endif
    float om[NL][16];                 // 1 - H_l^2 of this wave's blocks, from the forward to the backward phases
    for (int it = 0;; ++it) {
        const int tile = s_tile[it & 3];
        if (tile >= n_tiles) break;
#ifdef K7W_STAMPS
        wst[21] += 1;                    // tiles
#endif
        const int tile3 = s_tile[(it + 3) & 3];
        int ln = lane;
        asm volatile("" : "+v"(ln));          // opaque per-tile copy: LDS addresses are re-derived inside the phases, not hoisted and spilled
        {
            int wz = 0;                        // ... and the weight base (an opaque zero keeps it a scalar pointer per tile)
            asm volatile("" : "+s"(wz));
            wbase = wbase0 + wz;
            lane16 = ln * 16;
        }
        // ---- land the prefetched tile as bf16 planes
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's own pieces have landed in the staging area
        int tl = tid;
        asm volatile("" : "+v"(tl));
        if (vec4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tl + u * kThreads, r = e >> 5, c4 = (e & 31) * 4;
                const bool ok = (xok >> u) & 1u;
                const float4 v = *reinterpret_cast<const float4*>(sStage + e * 16);
                if (c4 < D) store_x4(sX + (c4 >> 6) * kXHalf, r, c4 & 63, ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tl + u * kThreads, r = e >> 7, c = e & 127;
                const float v = *reinterpret_cast<const float*>(sStage + e * 4);
                if (c < D) store_x1(sX + (c >> 6) * kXHalf, r, c & 63, ((xok >> u) & 1u) ? v : 0.0f);
            }
        }
        if (net == 0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = tl + u * kThreads;
                const float v = *reinterpret_cast<const float*>(sStageA + e * 4);
                sAct[(e >> 4) * LDO + (e & 15)] = ((xok >> (16 + u)) & 1u) ? v : 0.0f;
            }
        }
        if (tid < R) {
            sSrc[tid] = p_src;
            sRec[tid] = p_rec;
            sIdx[(it & 1) * R + tid] = n_ok ? n_raw : -1;
        }
        WBAR(0);

        // ---- forward: H_1 .. H_NL
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            f32x16 acc = zero16();
            WSUB0();
            if (cb < HB) {
                // (every chain below asks for the fragments of k-step ks + 1 BEFORE it issues the six products of k-step ks: with the
                // reads and the products of a pair of k-steps in one scheduling region the compiler put the reads first and the wave
                // waited out their latency in front of every pair -- 75-87 cycles per matrix instruction instead of 32,
                // tools/k7w_stamps.py)
                int lc = ln;
                asm volatile("" : "+v"(lc));       // (an opaque copy per chain: its fragment addresses are formed here, not at the top of the tile)
                if (l == 0) {
                    load_w_hi(0, 0, nksD);
                    Frag3 f0 = x_rows(sX, 0, lc), f1 = f0;          // two fragment sets take turns (no copies between them)
#pragma unroll
                    for (int ks = 0; ks < kOp3Ks; ks += 2) {
                        if (live<DK>(nksD, ks + 1)) f1 = x_rows(sX + ((ks + 1) >> 2) * kXHalf, (ks + 1) & 3, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<DK>(nksD, ks)) acc = mma32x3(f0, wfrag(ks), acc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<DK>(nksD, ks + 2)) f0 = x_rows(sX + ((ks + 2) >> 2) * kXHalf, (ks + 2) & 3, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<DK>(nksD, ks + 1)) acc = mma32x3(f1, wfrag(ks + 1), acc);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    load_w_hi(l, 0, nksH);
                    Frag3 f0 = f_cols<kFPlaneW>(sH(l - 1), 0, lc), f1 = f0;
#pragma unroll
                    for (int ks = 0; ks < kOp3Ks; ks += 2) {
                        if (live<HK>(nksH, ks + 1)) f1 = f_cols<kFPlaneW>(sH(l - 1), ks + 1, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks)) acc = mma32x3(f0, wfrag(ks), acc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks + 2)) f0 = f_cols<kFPlaneW>(sH(l - 1), ks + 2, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks + 1)) acc = mma32x3(f1, wfrag(ks + 1), acc);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#ifdef K7W_STAMPS
            { float sink = acc[0] + acc[15]; asm volatile("" :: "v"(sink)); }      // the chain has drained
#endif
            WSUB(l == 0 ? 24 : 28);
            if (l == 0) {
                // the next tile's rows, behind this tile's math.  Requested HERE, behind layer 1's products: the wait for their weight
                // slice (requested in the previous trip of the loop) is a vmcnt(0), and ahead of it these gathers' whole HBM latency
                // sat in every tile (tools/k7w_stamps.py: F1 took 8.1 k cycles for its 24 matrix instructions)
                prefetch(sIdx + ((it + 1) & 1) * R);
                prefetch_idx(a, n_tiles, tile3, n_ok, n_raw);
            }
            WSUB(25);
            if (cb < HB) {
                // the slice used next: the following layer's forward copy, or (behind the last layer) the top layer's backward copy
                if (l + 1 < NL) load_w(l + 1, 0, nksH);
                else if (NL > 1) load_w(NL - 1, 1, nksH);
                tanh_store<kFPlaneW>(sH(l), cb * 32, acc, sB[l * HPW + cb * 32 + (ln & 31)], ln, om[l]);
            }
            WSUB(l == 0 ? 26 : 29);
            WBAR(1 + l);
        }
        if (cb < 2) {   // head: 16 rows per wave on 16x16x32
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                if (ks < nks2H)
                    acc = mma16x3(f_cols16<kFPlaneW>(sH(NL - 1), 16 * cb, ks, ln),
                                  plain_rows(sW3, kW3RowW, kW3PlaneW, ln & 15, 32 * ks + 8 * (ln >> 4)), acc);
            const int col = ln & 15;
            const float bias = sB3[col];
#pragma unroll
            for (int e = 0; e < 4; ++e) sOut[(cb * 16 + 4 * (ln >> 4) + e) * LDO + col] = acc[e] + bias;
        }
        WBAR(4);
        int tile4 = 0;
        if (tid == 0) tile4 = tile_queue_next(queue, tile);

        // ---- loss lanes: this net's half of the PPO terms; head outputs become their gradients, fp32 (column sums) and as a
        // bf16-plane image (the two products below).  SIXTEEN lanes per row (lane k = head output k; rows tid >> 4 and + 16), the
        // sums over the outputs by butterfly inside the 16 lanes: as one lane per row walking its outputs, this phase was 6.2 k
        // cycles of a 51.6 k-cycle tile with 224 of the workgroup's threads waiting (tools/k7w_stamps.py)
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {      // (not unrolled: two passes' temporaries at once cost the 3-layer build 130 spilled registers)
            const int row = lrow + 16 * pass;
            float* const out = sOut + row * LDO;
            const bool live = sSrc[row] >= 0;
            const float4 rc = sRec[row];
            const float o_k = out[k16];
            float g_out = 0.0f;                       // d loss / d head output k of this row
            if (net == 1) {
                if (k16 == 0 && live) {
                    const PpoSample t = ppo_sample(rc.x, rc.x, rc.y, o_k, rc.w, rc.z, mean, denom, invM, a.h);
                    l_a += t.vl;
                    g_out = t.g_v;
                    g_b3c += t.g_v;
                }
            } else if (a.continuous) {
                const float zk = sAct[row * LDO + k16] - o_k;
                const float logp = row16_sum(k16 < A ? gauss_logp_ivar(zk, my_ivar, my_ls) : 0.0f);
                const PpoSample t = ppo_sample(logp, rc.x, rc.y, rc.w, rc.w, rc.z, mean, denom, invM, a.h);
                if (live) {
                    if (k16 == 0) { l_a += t.pg; l_b += ent_c; l_c += t.okl; l_d += t.kl; l_e += t.cf; }
                    if (k16 < A) {
                        g_out = gauss_dmu(t.g_logp, zk, my_ivar);
                        sDls[row * LDO + k16] = gauss_dls(t.g_logp, zk, my_ivar, g_ent);
                    }
                } else {
                    sDls[row * LDO + k16] = 0.0f;
                }
            } else {
                const bool in = k16 < A;
                const float mx = row16_max(in ? o_k : -3.0e38f);
                const float se = row16_sum(in ? expf(o_k - mx) : 0.0f);
                const float lse = mx + logf(se);
                const int ai = (int)sAct[row * LDO];
                const float lpk = o_k - lse, pk = in ? expf(lpk) : 0.0f;
                const float ent = -row16_sum(in ? pk * lpk : 0.0f);
                const float logp = row16_sum(in && k16 == ai ? lpk : 0.0f);
                const PpoSample t = ppo_sample(logp, rc.x, rc.y, rc.w, rc.w, rc.z, mean, denom, invM, a.h);
                if (live) {
                    if (k16 == 0) { l_a += t.pg; l_b += ent; l_c += t.okl; l_d += t.kl; l_e += t.cf; }
                    if (in) g_out = cat_dlogit(t.g_logp, k16 == ai, pk, lpk, ent, g_ent);
                }
                sDls[row * LDO + k16] = 0.0f;
            }
            out[k16] = g_out;
            store_plain1(sDo, kDoRowW, kDoPlaneW, k16, row, g_out);
        }
        WBAR(5);

        // ---- head backward: column sums (d b3, d logstd), dH_NL -> dZ_NL (in place), dW3
        if (net == 0 && w == 3 && lane < 2 * AP) g_head += head_colsum(sOut, sDls, lane);
        if (cb < HB) {
            char* const HL = sH(NL - 1);
            f32x16 acc = zero16();
            acc = mma32x3(plain_cols(sDo, kDoRowW, kDoPlaneW, 0, 0, ln), plain_cols(sW3, kW3RowW, kW3PlaneW, 0, cb * 32, ln), acc);
            {
                const Frag3 da = plain_rows(sDo, kDoRowW, kDoPlaneW, ln & 15, 8 * (ln >> 4));
#pragma unroll
                for (int q = 0; q < 2; ++q) gW3[q] = mma16x3(da, f_rows16<kFPlaneW>(HL, cb * 32 + 16 * q, ln), gW3[q]);
            }
            float colsum = dz_from_regs<kFPlaneW>(HL, cb * 32, acc, om[NL - 1], ln);
            colsum += __shfl_xor(colsum, 32, kWave);
            gb[NL - 1] += colsum;
        }
        WBAR(6);
        // ---- hidden layers, top down: dW_l, dH_{l-1} -> dZ_{l-1} (in place)
#pragma unroll
        for (int l = NL - 1; l >= 1; --l) {
            if (cb < HB) {
                const char* const dZ = sH(l);
                char* const Hp = sH(l - 1);
                load_w_hi(l, 1, nksH);                      // (behind the dW chains below)
                int lc = ln;
                asm volatile("" : "+v"(lc));
                {   // dW_l: eight (k-step, out-block) products, the next one's dZ fragment (and the next k-step's H fragment) asked for first
                    Frag3 hb0 = f_rows<kFPlaneW>(Hp, cb * 32, 0, lc), hb1 = hb0;
                    Frag3 d0 = f_rows<kFPlaneW>(dZ, 0, 0, lc), d1 = d0;
#pragma unroll
                    for (int q = 0; q < 8; q += 2) {            // q = 4 ks + ob
                        if (live<HBK>(HB, (q + 1) & 3)) d1 = f_rows<kFPlaneW>(dZ, ((q + 1) & 3) * 32, (q + 1) >> 2, lc);
                        if (q == 2) hb1 = f_rows<kFPlaneW>(Hp, cb * 32, 1, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HBK>(HB, q & 3)) gW[l][q & 3] = mma32x3(d0, q < 4 ? hb0 : hb1, gW[l][q & 3]);
                        __builtin_amdgcn_sched_barrier(0);
                        if (q + 2 < 8 && live<HBK>(HB, (q + 2) & 3)) d0 = f_rows<kFPlaneW>(dZ, ((q + 2) & 3) * 32, (q + 2) >> 2, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HBK>(HB, (q + 1) & 3)) gW[l][(q + 1) & 3] = mma32x3(d1, q < 4 ? hb0 : hb1, gW[l][(q + 1) & 3]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                f32x16 acc = zero16();
                {
                    Frag3 f0 = f_cols<kFPlaneW>(dZ, 0, lc), f1 = f0;
#pragma unroll
                    for (int ks = 0; ks < kOp3Ks; ks += 2) {
                        if (live<HK>(nksH, ks + 1)) f1 = f_cols<kFPlaneW>(dZ, ks + 1, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks)) acc = mma32x3(f0, wfrag(ks), acc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks + 2)) f0 = f_cols<kFPlaneW>(dZ, ks + 2, lc);
                        __builtin_amdgcn_sched_barrier(0);
                        if (live<HK>(nksH, ks + 1)) acc = mma32x3(f1, wfrag(ks + 1), acc);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (l - 1 >= 1) load_w(l - 1, 1, nksH);
                else load_w(0, 0, nksD);                    // layer 1's forward slice for the next tile
                float colsum = dz_from_regs<kFPlaneW>(Hp, cb * 32, acc, om[l - 1], ln);
                colsum += __shfl_xor(colsum, 32, kWave);
                gb[l - 1] += colsum;
            }
            WBAR(6 + l);
        }
        // ---- dW_1: this wave's 32 state columns against every out-block
        if (cb < DB) {
            const char* const dZ = sH(0);
            int lc = ln;
            asm volatile("" : "+v"(lc));
            Frag3 xb0 = x_cols(sX + (cb >> 1) * kXHalf, 0, (cb & 1) * 32, lc), xb1 = xb0;
            Frag3 d0 = f_rows<kFPlaneW>(dZ, 0, 0, lc), d1 = d0;
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                if (live<HBK>(HB, (q + 1) & 3)) d1 = f_rows<kFPlaneW>(dZ, ((q + 1) & 3) * 32, (q + 1) >> 2, lc);
                if (q == 2) xb1 = x_cols(sX + (cb >> 1) * kXHalf, 1, (cb & 1) * 32, lc);
                __builtin_amdgcn_sched_barrier(0);
                if (live<HBK>(HB, q & 3)) gW[0][q & 3] = mma32x3(d0, q < 4 ? xb0 : xb1, gW[0][q & 3]);
                __builtin_amdgcn_sched_barrier(0);
                if (q + 2 < 8 && live<HBK>(HB, (q + 2) & 3)) d0 = f_rows<kFPlaneW>(dZ, ((q + 2) & 3) * 32, (q + 2) >> 2, lc);
                __builtin_amdgcn_sched_barrier(0);
                if (live<HBK>(HB, (q + 1) & 3)) gW[0][(q + 1) & 3] = mma32x3(d1, q < 4 ? xb0 : xb1, gW[0][(q + 1) & 3]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (tid == 0) s_tile[it & 3] = tile4;
        WBAR(9);
    }

#ifdef K7W_STAMPS
    if (tid == 0) {
        wst[22] = __builtin_readcyclecounter() - wt_entry;     // entry to the end of the tile loop
#pragma unroll
        for (int k = 0; k < 32; ++k) g_k7w_stamps[blockIdx.x][k] = wst[k];
    }
#endif
    // ---- this workgroup's half of the pair's slab
    float* slab = a.slabs + (size_t)pair * a.L.n_params;
    {
        const int col = cb * 32 + (lane & 31);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int in_dim = l == 0 ? D : Hd;
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) {
                if (ob < HB && col < in_dim) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int o = ob * 32 + acc_row(e, lane);
                        if (o < Hd) slab[a.L.w[net][l] + o * in_dim + col] = gW[l][ob][e];
                    }
                }
            }
            if (lane < 32 && col < Hd) slab[a.L.b[net][l] + col] = gb[l];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {       // 16x16 accumulator layout: row = head output, col = hidden unit
            const int o = 4 * (lane >> 4) + e, c = cb * 32 + (lane & 15);
            if (o < out_dim && cb < HB) {
                if (c < Hd) slab[a.L.w[net][NL] + o * Hd + c] = gW3[0][e];
                if (c + 16 < Hd) slab[a.L.w[net][NL] + o * Hd + c + 16] = gW3[1][e];
            }
        }
    }
    if (net == 0 && w == 3) slab_head_sums<NL>(slab, a, lane, g_head);
    {   // the loss sums and the critic's bias gradient sit on lane 0 of every DPP row of all four waves
        __shared__ double s_fin[kThreads / kWave][6];
        double v6[6] = {l_a, l_b, l_c, l_d, l_e, (double)g_b3c};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double x = k16 == 0 ? v6[q] : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, kWave);
            if (lane == 0) s_fin[w][q] = x;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) v6[q] = ((s_fin[0][q] + s_fin[1][q]) + s_fin[2][q]) + s_fin[3][q];
            loss_record<NL>(a, slab, pair, net, v6, (float)v6[5], mean, s_std);
        }
    }
}

}  // namespace

namespace aurppo_mlp {

int launch_mlpw3_prep(const WideArgs& a, int num_layers, int M, int sb, double* stats, unsigned* tile_counter, unsigned short* wop3, hipStream_t s) {
    hipLaunchKernelGGL(k_mlpw3_prep, dim3(sb + 96), dim3(256), 0, s, a.params, a.L, num_layers, a.D, a.Hd, wop3, a.rec, a.rec_stride, a.idx, M,
                       reinterpret_cast<double (*)[2]>(stats), sb, tile_counter);
    AURPPO_LAUNCH_CHECK("k_mlpw_prep");
    return AURPPO_OK;
}

// k_mlpw3_step.  Hidden layers of 113..128 / 81..96 units over <= 64 / <= 128 state floats: the builds whose matrix chains have
// compile-time trip counts; every other width runs the build with run-time counts
int launch_mlpw3_step(const WideArgs& a, int num_layers, int grid, hipStream_t s) {
    const int hk = a.Hd > 112 ? 8 : ((a.Hd > 80 && a.Hd <= 96) ? 6 : 0);
    const bool d64 = a.D <= 64;
    return wide_with_nl(num_layers, [&](auto n) {
        auto go = [&](auto h, auto d) {
            return wide_launch<k_mlpw3_step<decltype(n)::value, decltype(h)::value, decltype(d)::value>>("k_mlpw_step", grid, w3::kBytes, s, a);
        };
        using I0 = std::integral_constant<int, 0>;
        using I4 = std::integral_constant<int, 4>;
        using I6 = std::integral_constant<int, 6>;
        using I8 = std::integral_constant<int, 8>;
        if (hk == 8) return d64 ? go(I8{}, I4{}) : go(I8{}, I8{});
        if (hk == 6) return d64 ? go(I6{}, I4{}) : go(I6{}, I8{});
        return go(I0{}, I0{});
    });
}

}  // namespace aurppo_mlp

#ifdef K7W_STAMPS
extern "C" int aurppo_k7w_stamps_read(unsigned long long* host_out) {      // (kMaxSlabs, 32); diagnostic build only
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_k7w_stamps), sizeof(unsigned long long) * kMaxSlabs * 32) == hipSuccess ? 0 : -1;
}
#endif
