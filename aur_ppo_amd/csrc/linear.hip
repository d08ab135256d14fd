// nn.Linear on K11's arithmetic (conv.hip: fp32 products as six bf16 MFMAs, bf3_gemm.h), for the MLP shapes the fused K7 / K7w steps do
// not cover (src/nets/nets.py:21-27,33-39,45-51 with hidden_dim > 128): the product k_linear / k_linear_tail, forward and input
// gradient, and the weight gradient k_linear_wgrad / k_linear_wgrad_tail.  The filter's operand copy (k_conv_prep, k_linear_prep_tail)
// and the fold of the weight gradient's slices (k_fold_slices*) are conv.hip's kernels, reached through common.h.
//
// The product: y (M, N) = x (M, K) . B (K, N), x row-major -- a 1 x 1 "convolution" whose pixels are the minibatch's rows.  Same
// filter staging and matrix loop as k_conv3x3; the A values of a k-step are 32 contiguous bytes per lane (two 16-byte loads), and
// the accumulator's lane-per-column layout already matches the row-major output (32 lanes = 128 contiguous bytes): no LDS tile.
#pragma clang fp contract(fast)
#include "bf3_gemm.h"
#include "common.h"

using namespace bf3;

namespace {

struct LinArgs {
    const float* x;                  // (M, K)
    const unsigned short* wop;       // [n-block][k-step][plane][lane][8]
    float* y;                        // (M, N)
    const float* bias;               // (n_bias,) or nullptr
    long long M;
    int K, N, n_mb;
    int act;                         // 0: none, 1: tanh (1 - 2 / (e^{2x} + 1), as the fused MLP steps form it)
                                     // 2 (GATE builds): y = acc * (1 - h * h), tanh' of the layer below from its output h
    const int32_t* rows;             // ROWS builds: (M,) lane row m reads x row rows[m] (the minibatch index); y stays in minibatch order
    const float* h;                  // GATE builds: (M, N), read at the address the store uses
    int n_bias;                      // N, or fewer: the columns from n_bias on add 0 (a product that runs wider than its layer, common.h)
};

// ROWS (layer 0 of the layered PPO step, hip_ops.mlp_layered_step: x through the minibatch index) and GATE (its input gradients:
// tanh' of the layer below in the epilogue) are template parameters, so the plain instantiations keep their instruction streams.
// KTAIL (k_linear_tail: K is no multiple of 16 -- layer 0 of a policy whose state is 3, 11, 17, 376 floats wide): KS = ceil(K / 16)
// k-steps against an operand copy whose columns >= K are zero planes (k_linear_prep_tail).  A row is K floats and nothing more: it
// starts at a 4-byte boundary, what follows it is another row, somebody else's memory or an unmapped page.  So every k-step's A values
// are eight dword loads per lane, each one issued only where its column is < K, and the columns >= K enter split3 as a selected 0.
// Every product kernel below shares one body text, linear_body.h (it says why a text): KTAIL, MB (32-row blocks per wave) and `wg` (the
// workgroup's index inside its product's grid) are names of the including kernel.
template <int NB, bool ROWS = false, bool GATE = false>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear(const LinArgs a) {
    constexpr bool KTAIL = false, GRAD = GATE;
    constexpr int MB = kMB;
    const unsigned wg = blockIdx.x;
#include "linear_body.h"
}
template <int NB, bool ROWS>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_tail(const LinArgs a) {
    constexpr bool GATE = false, GRAD = false, KTAIL = true;
    constexpr int MB = kMB;
    const unsigned wg = blockIdx.x;
#include "linear_body.h"
}
// GRAD: the product is an input gradient (mode 1), whose k-steps change sign in another order in every other block of 32 rows
// (linear_body.h says why).  The GATE builds above are input gradients already; this overload is the plain mode-1 product.
template <int NB, bool ROWS, bool GATE, bool GRAD>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear(const LinArgs a) {
    static_assert(GRAD && !ROWS && !GATE, "the plain input gradient");
    constexpr bool KTAIL = false;
    constexpr int MB = kMB;
    const unsigned wg = blockIdx.x;
#include "linear_body.h"
}

// ---- the small-M builds of the forward product: the same body text at MB = 1 (linear_body.h says why the bits are k_linear's).  New
// templates, not parameters on the templates above: those keep their symbols.  k_linear_small / k_linear_small_tail: one product.
// k_linear_pair / k_linear_pair_tail: the same-shaped product of two nets (the layered rollout's actor and critic, layer by layer) in
// one launch -- workgroups [0, per_net) are net 0's grid, [per_net, 2 per_net) net 1's; the net's four pointers are selected once,
// ahead of the body, so the k loop has no branch on the net.  The two x pointers may be equal (layer 0: both nets read the observations).
struct LinPairArgs {
    const float* x[2];               // (M, K) each
    const unsigned short* wop[2];    // each net's operand copy, the layout above
    float* y[2];                     // (M, N) each
    const float* bias[2];            // (n_bias,) or nullptr
    long long M;
    int K, N, n_mb, n_bias, act;
    unsigned per_net;                // workgroups of one net's product
};
template <int NB>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_small(const LinArgs a) {
    constexpr bool KTAIL = false, ROWS = false, GATE = false, GRAD = false;
    constexpr int MB = 1;
    const unsigned wg = blockIdx.x;
#include "linear_body.h"
}
template <int NB>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_small_tail(const LinArgs a) {
    constexpr bool KTAIL = true, ROWS = false, GATE = false, GRAD = false;
    constexpr int MB = 1;
    const unsigned wg = blockIdx.x;
#include "linear_body.h"
}
__device__ __forceinline__ LinArgs pair_net_args(const LinPairArgs& p, unsigned net) {
    LinArgs a;
    a.x = net ? p.x[1] : p.x[0];
    a.wop = net ? p.wop[1] : p.wop[0];
    a.y = net ? p.y[1] : p.y[0];
    a.bias = net ? p.bias[1] : p.bias[0];
    a.M = p.M; a.K = p.K; a.N = p.N; a.n_mb = p.n_mb; a.n_bias = p.n_bias; a.act = p.act;
    a.rows = nullptr; a.h = nullptr;
    return a;
}
template <int NB>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_pair(const LinPairArgs p) {
    constexpr bool KTAIL = false, ROWS = false, GATE = false, GRAD = false;
    constexpr int MB = 1;
    const unsigned net = blockIdx.x >= p.per_net ? 1u : 0u, wg = blockIdx.x - net * p.per_net;
    const LinArgs a = pair_net_args(p, net);
#include "linear_body.h"
}
template <int NB>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_pair_tail(const LinPairArgs p) {
    constexpr bool KTAIL = true, ROWS = false, GATE = false, GRAD = false;
    constexpr int MB = 1;
    const unsigned net = blockIdx.x >= p.per_net ? 1u : 0u, wg = blockIdx.x - net * p.per_net;
    const LinArgs a = pair_net_args(p, net);
#include "linear_body.h"
}

// ---- nn.Linear's weight gradient on the same arithmetic: dW (N, K) = dY^T (N, M) . X (M, K), both operands row-major with the
// minibatch's rows as the product's inner dimension.  Both operands change every k-step, so both are split; to split every
// element once per WORKGROUP (not once per wave that uses it) the workgroup stages 32 rows of its 128 dY columns and its 128 X
// columns as bf16-plane X images in LDS (bf16x3.h: 8-byte stores along a row, fragments by transposed reads across rows -- the
// images k_mlp_step3 lands its observation rows in), and its four waves each form a 64 x 64 quarter of the 128 x 128 tile.
// The inner dimension is cut into S slices: partial[s] (N, K) per slice, summed by the caller in fixed order (deterministic).
struct WgradArgs {
    const float* dy;                 // (M, N)
    const float* x;                  // (M, K)
    float* part;                     // (S, N, K)
    long long M;
    int N, K, rows_per_slice, n_tiles_n, n_tiles_k;
    const int32_t* rows;             // ROWS builds: (M,) row m of the product reads x row rows[m]; dy stays in minibatch order
    double* bpart;                   // BIAS builds: (S, N) the slices' column sums of dy, behind `part` (the other builds never read it)
};

// KTAIL (k_linear_wgrad_tail: K is no multiple of 4 -- layer 0's weight gradient at a ragged state width): an X row is K floats
// at a 4-byte boundary, so its piece of a chunk is four dword loads, each issued only where its column is < K; the columns >= K
// are staged as a selected 0 (and the stores to `part` leave them out, as they always did).
template <bool ROWS = false>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_wgrad(const WgradArgs a) {
    constexpr bool KTAIL = false, BIAS = false;
#include "linear_wgrad_body.h"
}
template <bool ROWS>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_wgrad_tail(const WgradArgs a) {
    constexpr bool KTAIL = true, BIAS = false;
#include "linear_wgrad_body.h"
}
// The builds that also leave the layer's bias gradient, the column sums of dy (linear_wgrad_body.h).  They are overloads with a
// second template parameter, not a defaulted one on the templates above: those keep their symbols and their instruction streams.
template <bool ROWS, bool BIAS>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_wgrad(const WgradArgs a) {
    constexpr bool KTAIL = false;
#include "linear_wgrad_body.h"
}
template <bool ROWS, bool BIAS>
__global__ __launch_bounds__(kConvThreads, 2) void k_linear_wgrad_tail(const WgradArgs a) {
    constexpr bool KTAIL = true;
#include "linear_wgrad_body.h"
}

}  // namespace

// The two halves of a product, host side: the filter into operand order (linear_prep, conv.hip) and a k_linear* kernel from an operand
// copy that exists.  linear_impl and the small / paired entries do both per call; the layered rollout step (layered.hip) builds the
// copies once per rollout and comes in through aurppo_linear_forward.
// linear_launch is the second half for every product on checked operands: `small` the tile (k_linear's 256 rows x NB <= 4 blocks, or
// the small-M tile with its NB from bf3_small_grid), `nets` same-shaped products in ONE launch (2: the small tile only, k_linear_pair)
// from ops[0 .. nets).  rows, h, grad: the large tile's index, gate and input-gradient builds.
static int linear_launch(bool small, int nets, const LinOps* ops, int act, long long M, int K, int N, hipStream_t s,
                         const int32_t* rows = nullptr, const float* h = nullptr, bool grad = false, int n_bias = 0) {
    const Bf3Grid gr = small ? bf3_small_grid(M, N, nets) : bf3_grid(M, N);
    const long long per_net = gr.n_mb * gr.n_ng;
    AURPPO_REQUIRE(per_net * nets < (1ll << 31), AURPPO_ESHAPE, "%s: grid too large", small ? "aurppo_linear_small_bias_act_f32" : "aurppo_linear_f32");
    AURPPO_REQUIRE(K % 16 == 0 || !(h || grad), AURPPO_ESHAPE, "aurppo_linear_f32: the input gradient's inner dimension %d (a multiple of 16)", K);
    AURPPO_REQUIRE(!(grad && rows), AURPPO_EINVAL, "aurppo_linear_f32: an input gradient through an index");
    LinArgs a;
    LinPairArgs p;
    for (int net = 0; net < nets; ++net) {
        p.x[net] = ops[net].x; p.wop[net] = reinterpret_cast<const unsigned short*>(ops[net].wop); p.y[net] = ops[net].y; p.bias[net] = ops[net].bias;
    }
    a.x = p.x[0]; a.wop = p.wop[0]; a.y = p.y[0]; a.bias = p.bias[0]; a.rows = rows; a.h = h;
    a.M = p.M = M; a.K = p.K = K; a.N = p.N = N; a.n_mb = p.n_mb = (int)gr.n_mb; a.act = p.act = act;
    a.n_bias = p.n_bias = n_bias > 0 && n_bias < N ? n_bias : N;
    p.per_net = (unsigned)per_net;
    const dim3 g((unsigned)(per_net * nets)), blk(kConvThreads);
    const bool tail = K % 16 != 0, nb2 = gr.NB == 2;
    if (nets == 2) {
        if (tail && nb2) hipLaunchKernelGGL(k_linear_pair_tail<2>, g, blk, 0, s, p);
        else if (tail) hipLaunchKernelGGL(k_linear_pair_tail<1>, g, blk, 0, s, p);
        else if (nb2) hipLaunchKernelGGL(k_linear_pair<2>, g, blk, 0, s, p);
        else hipLaunchKernelGGL(k_linear_pair<1>, g, blk, 0, s, p);
        AURPPO_LAUNCH_CHECK("k_linear_pair");
    } else if (small) {
        if (tail && nb2) hipLaunchKernelGGL(k_linear_small_tail<2>, g, blk, 0, s, a);
        else if (tail) hipLaunchKernelGGL(k_linear_small_tail<1>, g, blk, 0, s, a);
        else if (nb2) hipLaunchKernelGGL(k_linear_small<2>, g, blk, 0, s, a);
        else hipLaunchKernelGGL(k_linear_small<1>, g, blk, 0, s, a);
        AURPPO_LAUNCH_CHECK("k_linear_small");
    } else {
        bf3_with_nb(gr.NB, [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            if (tail) {
                if (rows) hipLaunchKernelGGL((k_linear_tail<NB, true>), g, blk, 0, s, a);
                else hipLaunchKernelGGL((k_linear_tail<NB, false>), g, blk, 0, s, a);
            } else if (h) hipLaunchKernelGGL((k_linear<NB, false, true>), g, blk, 0, s, a);
            else if (grad) hipLaunchKernelGGL((k_linear<NB, false, false, true>), g, blk, 0, s, a);
            else if (rows) hipLaunchKernelGGL((k_linear<NB, true, false>), g, blk, 0, s, a);
            else hipLaunchKernelGGL(k_linear<NB>, g, blk, 0, s, a);
        });
        AURPPO_LAUNCH_CHECK("k_linear");
    }
    return AURPPO_OK;
}

// What every forward entry on operand copies refuses, once per call and under the entry's name `who`: `copy` is what the entry calls
// the memory behind ops[].wop, `others` whether the pointers that only the entry knows (its weights) are there.
static int linear_forward_check(const char* who, const char* copy, bool others, bool small, int nets, const LinOps* ops, int act,
                                long long M, int K, int N) {
    AURPPO_REQUIRE(nets == 1 || (nets == 2 && small), AURPPO_EINVAL, "%s: %d products in one launch", who, nets);
    AURPPO_REQUIRE(act == 0 || act == 1, AURPPO_EINVAL, "%s: act %d", who, act);
    bool there = others, aligned = true;
    for (int net = 0; net < nets; ++net) {
        there = there && ops[net].x && ops[net].wop && ops[net].y;
        aligned = aligned && aligned_to(ops[net].x, 16) && aligned_to(ops[net].wop, 16);
    }
    AURPPO_REQUIRE(there, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(M > 0 && K > 0 && N > 0, AURPPO_ESHAPE, "%s: M=%lld, inner dimension %d, %d columns", who, M, K, N);
    AURPPO_REQUIRE(aligned, AURPPO_EINVAL, "%s: x / %s not 16-byte aligned", who, copy);
    return AURPPO_OK;
}

// mode 0: y (M, N_w) = x (M, K_w) . w (N_w, K_w)^T      -- nn.Linear without its bias; any K_w >= 1 (no multiple of 16: the tail builds)
// mode 1: y (M, K_w) = x (M, N_w) . w (N_w, K_w)         -- the gradient with respect to the input (x is dY); N_w a multiple of 16
// wop_ws: aurppo_conv3x3_wop_bytes(product's K, product's N) / 9 bytes suffice; the same function's size is accepted.
// Kg, Ng (0: the weight's own): the product's dimensions where it runs wider than its weight (common.h) -- x, y and h are then (M, Kg)
// and (M, Ng) planes, the copy comes from linear_prep_pad and the bias (mode 0) is added to the weight's N_w columns alone.
static int linear_impl(const float* x, const float* w, const float* bias, int act, float* y, long long M, int K_w, int N_w, int mode,
                       void* wop_ws, void* stream, const int32_t* rows = nullptr, const float* h = nullptr, int Kg = 0, int Ng = 0) {
    AURPPO_REQUIRE(x && w && y && wop_ws, AURPPO_EINVAL, "aurppo_linear_f32: null pointer");
    AURPPO_REQUIRE(mode == 0 || mode == 1, AURPPO_EINVAL, "aurppo_linear_f32: mode %d", mode);
    const int K_own = mode == 0 ? K_w : N_w, N_own = mode == 0 ? N_w : K_w;
    const int K = Kg ? Kg : K_own, N = Ng ? Ng : N_own;
    const bool pad = K != K_own || N != N_own;
    AURPPO_REQUIRE(M > 0 && K_own > 0 && N_own > 0 && K >= K_own && N >= N_own && (mode == 0 || K % 16 == 0), AURPPO_ESHAPE,
                   "aurppo_linear_f32: M=%lld, inner dimension %d (mode 1: a multiple of 16), %d columns", M, K, N);
    AURPPO_REQUIRE(aligned_to(x, 16) && aligned_to(wop_ws, 16), AURPPO_EINVAL, "aurppo_linear_f32: x / workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned short* wop = reinterpret_cast<unsigned short*>(wop_ws);
    if (const int rc = pad ? linear_prep_pad(w, K_w, N_w, mode, K, N, wop, s) : linear_prep(w, K_w, N_w, mode, wop, s)) return rc;
    const LinOps ops = {x, wop, bias, y};
    return linear_launch(false, 1, &ops, act, M, K, N, s, rows, h, mode == 1, N_own);
}
int linear_product(const float* x, const float* w, const float* bias, int act, float* y, long long M, int K_w, int N_w, int mode, int Kg,
                   int Ng, void* wop_ws, void* stream, const int32_t* rows, const float* h) {
    AURPPO_REQUIRE(act == (h ? 2 : 1) && (h != nullptr) == (mode == 1), AURPPO_EINVAL, "aurppo_linear_f32: act %d in mode %d", act, mode);
    return linear_impl(x, w, bias, act, y, M, K_w, N_w, mode, wop_ws, stream, rows, h, Kg, Ng);
}

extern "C" int aurppo_linear_f32(const float* x, const float* w, float* y, long long M, int K_w, int N_w, int mode, void* wop_ws,
                                 void* stream) {
    return linear_impl(x, w, nullptr, 0, y, M, K_w, N_w, mode, wop_ws, stream);
}

// y (M, N_w) = act(x (M, K_w) . w (N_w, K_w)^T + bias): nn.Linear with its bias and, act = 1, the nn.Tanh behind it
// (src/nets/nets.py:21-27: every hidden layer of the reference's MLPs) in the product's epilogue.
extern "C" int aurppo_linear_bias_act_f32(const float* x, const float* w, const float* bias, float* y, long long M, int K_w, int N_w,
                                          int act, void* wop_ws, void* stream) {
    AURPPO_REQUIRE(act == 0 || act == 1, AURPPO_EINVAL, "aurppo_linear_bias_act_f32: act %d", act);
    return linear_impl(x, w, bias, act, y, M, K_w, N_w, 0, wop_ws, stream);
}

// The same with lane row m reading x row rows[m] (rows == NULL: aurppo_linear_bias_act_f32): the K3 gather of the minibatch's
// observations (src/ppo.py:219-220) rides in the first layer's product.  Every rows[m] must name a row of x.
extern "C" int aurppo_linear_rows_bias_act_f32(const float* x, const int32_t* rows, const float* w, const float* bias, float* y,
                                               long long M, int K_w, int N_w, int act, void* wop_ws, void* stream) {
    AURPPO_REQUIRE(act == 0 || act == 1, AURPPO_EINVAL, "aurppo_linear_rows_bias_act_f32: act %d", act);
    return linear_impl(x, w, bias, act, y, M, K_w, N_w, 0, wop_ws, stream, rows);
}

// out (M, K_w) = (gz (M, N_w) . w (N_w, K_w)) * (1 - h * h), h (M, K_w): the input gradient of a hidden layer with tanh' of the
// layer below in the epilogue (what autograd's mm + tanh_backward leave); out may be h itself.
extern "C" int aurppo_linear_dx_tanh_f32(const float* gz, const float* w, const float* h, float* out, long long M, int K_w, int N_w,
                                         void* wop_ws, void* stream) {
    AURPPO_REQUIRE(h, AURPPO_EINVAL, "aurppo_linear_dx_tanh_f32: null pointer");
    return linear_impl(gz, w, nullptr, 2, out, M, K_w, N_w, 1, wop_ws, stream, nullptr, h);
}

// ---- prepared weights for the layered rollout step (layered.hip).  Bytes of one forward operand copy: the blocks k_conv_prep writes and one group of slack, as a workgroup reads whole groups.
size_t aurppo_linear_wop_bytes(int K, int N) { return (size_t)((N + 31) / 32 + kNBW) * (size_t)((K + 15) / 16) * 3 * 1024; }

// y (M, N) = act(x (M, K) . B + bias) for each of ops[0 .. nets), from the operand copies of (N, K) weights: the forward products without
// their k_conv_prep launch, on the large tile or the small one (common.h)
int aurppo_linear_forward(const char* who, bool small, int nets, const LinOps* ops, int act, long long M, int K, int N, void* stream,
                          int n_bias) {
    if (const int rc = linear_forward_check(who, "operand copy", true, small, nets, ops, act, M, K, N)) return rc;
    return linear_launch(small, nets, ops, act, M, K, N, (hipStream_t)stream, nullptr, nullptr, false, n_bias);
}

// aurppo_linear_bias_act_f32 on the small tile, whatever M: same argument list, same checks, same bits
extern "C" int aurppo_linear_small_bias_act_f32(const float* x, const float* w, const float* bias, float* y, long long M, int K_w, int N_w,
                                                int act, void* wop_ws, void* stream) {
    const LinOps ops = {x, wop_ws, bias, y};
    if (const int rc = linear_forward_check("aurppo_linear_small_bias_act_f32", "workspace", w != nullptr, true, 1, &ops, act, M, K_w, N_w))
        return rc;
    if (const int rc = linear_prep(w, K_w, N_w, 0, reinterpret_cast<unsigned short*>(wop_ws), (hipStream_t)stream)) return rc;
    return linear_launch(true, 1, &ops, act, M, K_w, N_w, (hipStream_t)stream);
}

// Both nets' operand copies, one behind the other: 2 x aurppo_linear_wop_bytes (a multiple of 1 KB, so the second is aligned too)
extern "C" size_t aurppo_linear_pair_wop_bytes(int K_w, int N_w) {
    if (K_w <= 0 || N_w <= 0) return 0;
    return 2 * aurppo_linear_wop_bytes(K_w, N_w);
}
// yA = act(xA . wA^T + biasA) and yC = act(xC . wC^T + biasC), two (N_w, K_w) weights on the same M rows: two operand copies into
// wop_ws (aurppo_linear_pair_wop_bytes), then ONE launch of the paired small-tile product.  Each result is bit for bit what
// aurppo_linear_bias_act_f32 gives for its net.  xA may be xC.
extern "C" int aurppo_linear_pair_bias_act_f32(const float* xA, const float* xC, const float* wA, const float* wC, const float* biasA,
                                               const float* biasC, float* yA, float* yC, long long M, int K_w, int N_w, int act,
                                               void* wop_ws, void* stream) {
    char* const wopA = reinterpret_cast<char*>(wop_ws);
    char* const wopC = wopA ? wopA + aurppo_linear_wop_bytes(K_w, N_w) : nullptr;
    const LinOps ops[2] = {{xA, wopA, biasA, yA}, {xC, wopC, biasC, yC}};
    if (const int rc = linear_forward_check("aurppo_linear_pair_bias_act_f32", "workspace", wA && wC, true, 2, ops, act, M, K_w, N_w)) return rc;
    if (const int rc = linear_prep(wA, K_w, N_w, 0, reinterpret_cast<unsigned short*>(wopA), (hipStream_t)stream)) return rc;
    if (const int rc = linear_prep(wC, K_w, N_w, 0, reinterpret_cast<unsigned short*>(wopC), (hipStream_t)stream)) return rc;
    return linear_launch(true, 2, ops, act, M, K_w, N_w, (hipStream_t)stream);
}

// the weight gradient's slice count (slices_for, conv.hip, says how the slices are used)
static int linear_wgrad_slices(long long M, int N, int K) {
    const long long tiles = (long long)((N + 127) / 128) * ((K + 127) / 128);
    return slices_for(tiles, (M + 255) / 256);                // at least 8 chunks of 32 rows per slice
}
extern "C" size_t aurppo_linear_wgrad_ws_bytes(long long M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (size_t)linear_wgrad_slices(M, N, K) * (size_t)N * (size_t)K * sizeof(float) + 64;
}
// bytes of the (S, N, K) partial products, rounded to where the BIAS builds' (S, N) fp64 partial column sums begin
static size_t linear_wgrad_part_bytes(int S, int N, int K) { return ((size_t)S * (size_t)N * (size_t)K * sizeof(float) + 15) & ~(size_t)15; }
// The weight-gradient launches; db != nullptr: the BIAS builds and their fold (rows or K a multiple of 4: no plain BIAS tail build)
// Nr, Kr (0: N, K): dw is the (Nr, Kr) corner of the product, which ran on padded planes (common.h) -- the fold writes that corner alone
static int linear_wgrad_impl(const float* dy, const float* x, const int32_t* rows, float* dw, float* db, long long M, int N, int K,
                             void* ws, void* stream, int Nr = 0, int Kr = 0) {
    AURPPO_REQUIRE(dy && x && dw && ws, AURPPO_EINVAL, "aurppo_linear_wgrad_f32: null pointer");
    AURPPO_REQUIRE(M > 0 && N > 0 && K > 0 && N % 4 == 0, AURPPO_ESHAPE, "aurppo_linear_wgrad_f32: M=%lld N=%d (a multiple of 4) K=%d", M, N, K);
    if (!Nr) Nr = N;
    if (!Kr) Kr = K;
    AURPPO_REQUIRE(Nr > 0 && Nr <= N && Kr > 0 && Kr <= K, AURPPO_ESHAPE, "aurppo_linear_wgrad_f32: a %d x %d gradient out of %d x %d", Nr, Kr, N, K);
    AURPPO_REQUIRE(aligned_to(dy, 16) && aligned_to(x, 16) && aligned_to(ws, 16), AURPPO_EINVAL,
                   "aurppo_linear_wgrad_f32: operands / workspace not 16-byte aligned");
    const int S0 = linear_wgrad_slices(M, N, K);
    WgradArgs a;
    a.dy = dy; a.x = x; a.part = reinterpret_cast<float*>(ws); a.M = M; a.N = N; a.K = K; a.rows = rows;
    a.bpart = db ? reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + linear_wgrad_part_bytes(S0, N, K)) : nullptr;
    const long long rps = ((M + S0 - 1) / S0 + 31) / 32 * 32;           // whole 32-row chunks per slice
    const long long S = (M + rps - 1) / rps;
    AURPPO_REQUIRE(S >= 1 && S <= S0 && rps < (1ll << 30), AURPPO_ESHAPE, "aurppo_linear_wgrad_f32: slice size");
    a.rows_per_slice = (int)rps;
    a.n_tiles_n = (N + 127) / 128;
    a.n_tiles_k = (K + 127) / 128;
    const long long grid = (long long)a.n_tiles_n * a.n_tiles_k * S;
    AURPPO_REQUIRE(grid < (1ll << 31), AURPPO_ESHAPE, "aurppo_linear_wgrad_f32: grid too large");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g((unsigned)grid), blk(kConvThreads);
    const bool tail = K % 4 != 0;
    if (db && tail) hipLaunchKernelGGL((k_linear_wgrad_tail<true, true>), g, blk, 0, st, a);
    else if (db && rows) hipLaunchKernelGGL((k_linear_wgrad<true, true>), g, blk, 0, st, a);
    else if (db) hipLaunchKernelGGL((k_linear_wgrad<false, true>), g, blk, 0, st, a);
    else if (tail && rows) hipLaunchKernelGGL(k_linear_wgrad_tail<true>, g, blk, 0, st, a);
    else if (tail) hipLaunchKernelGGL(k_linear_wgrad_tail<false>, g, blk, 0, st, a);
    else if (rows) hipLaunchKernelGGL(k_linear_wgrad<true>, g, blk, 0, st, a);
    else hipLaunchKernelGGL(k_linear_wgrad<false>, g, blk, 0, st, a);
    AURPPO_LAUNCH_CHECK("k_linear_wgrad");
    if (Nr != N || Kr != K) return fold_slices_pad_launch(a.part, (int)S, N, K, Nr, Kr, dw, a.bpart, db, st);
    return fold_slices_launch(a.part, (int)S, (long long)N * K, dw, a.bpart, N, db, st);
}
int linear_wgrad_product(const float* dy, const float* x, const int32_t* rows, float* dw, float* db, long long M, int N, int K, int Nr, int Kr,
                         void* ws, void* stream) {
    AURPPO_REQUIRE(!db || (aligned_to(db, 4) && (rows || K % 4 == 0)), AURPPO_EINVAL, "aurppo_linear_wgrad_bias_f32: db not 4-byte aligned / K=%d", K);
    return linear_wgrad_impl(dy, x, rows, dw, db, M, N, K, ws, stream, Nr, Kr);
}
// dw (N, K) = dy (M, N)^T . x (M, K): nn.Linear's weight gradient (row-major fp32; N a multiple of 4, any K >= 1 -- no multiple of 4:
// the tail builds; 16-byte aligned operands)
extern "C" int aurppo_linear_wgrad_f32(const float* dy, const float* x, float* dw, long long M, int N, int K, void* ws, void* stream) {
    return linear_wgrad_impl(dy, x, nullptr, dw, nullptr, M, N, K, ws, stream);
}
// the same with row m of the product reading x row rows[m] (rows == NULL: the plain call); same slice rule, same workspace
extern "C" int aurppo_linear_wgrad_rows_f32(const float* dy, const float* x, const int32_t* rows, float* dw, long long M, int N, int K,
                                            void* ws, void* stream) {
    return linear_wgrad_impl(dy, x, rows, dw, nullptr, M, N, K, ws, stream);
}
// ... and with the layer's bias gradient db (N,) = the column sums of dy, taken in the product's kernel: the slices' partial sums
// (fp64) lie behind the partial products in the workspace
extern "C" size_t aurppo_linear_wgrad_bias_ws_bytes(long long M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = linear_wgrad_slices(M, N, K);
    return linear_wgrad_part_bytes(S, N, K) + (size_t)S * (size_t)N * sizeof(double) + 64;
}
extern "C" int aurppo_linear_wgrad_bias_f32(const float* dy, const float* x, const int32_t* rows, float* dw, float* db, long long M, int N,
                                            int K, void* ws, void* stream) {
    AURPPO_REQUIRE(db && aligned_to(db, 4), AURPPO_EINVAL, "aurppo_linear_wgrad_bias_f32: db null or not 4-byte aligned");
    AURPPO_REQUIRE(rows || K % 4 == 0, AURPPO_ESHAPE, "aurppo_linear_wgrad_bias_f32: K=%d (a multiple of 4 without rows)", K);
    return linear_wgrad_impl(dy, x, rows, dw, db, M, N, K, ws, stream);
}
