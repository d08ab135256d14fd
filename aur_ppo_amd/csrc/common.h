// Shared helpers for libaurppo_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/aurppo.h"

void aurppo_set_error(const char* fmt, ...);

#define AURPPO_HIP_TRY(expr)                                                   \
    do {                                                                       \
        hipError_t e__ = (expr);                                               \
        if (e__ != hipSuccess) {                                               \
            aurppo_set_error("%s failed: %s", #expr, hipGetErrorString(e__));  \
            return AURPPO_EHIP;                                                \
        }                                                                      \
    } while (0)

#define AURPPO_LAUNCH_CHECK(name)                                              \
    do {                                                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            aurppo_set_error("launch of %s failed: %s", name, hipGetErrorString(e__)); \
            return AURPPO_EHIP;                                                \
        }                                                                      \
    } while (0)

#define AURPPO_REQUIRE(cond, code, ...)                                        \
    do {                                                                       \
        if (!(cond)) {                                                         \
            aurppo_set_error(__VA_ARGS__);                                     \
            return (code);                                                     \
        }                                                                      \
    } while (0)

constexpr int kWave = 64;

// Per-device launch state (function attributes are per device; one process may drive several): slot of the calling
// thread's current device in small static tables.
constexpr int kMaxDevices = 16;
static inline int aurppo_device_slot() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
    return d;
}
// Launch of a kernel with dynamic LDS that may be above the default limit: the first launch per device sets the kernel's
// hipFuncAttributeMaxDynamicSharedMemorySize to lds_cap, whatever this launch needs; every launch asks for lds (<= lds_cap; most
// callers pass the same figure twice) and is checked under `name`.  Keyed on the kernel itself, so every instantiation owns its
// per-device flags.
template <auto Kernel, class Args>
int launch_dyn_lds(const char* name, int grid, int threads, size_t lds, size_t lds_cap, hipStream_t s, const Args& a) {
    static bool done[kMaxDevices] = {};
    const int dslot = aurppo_device_slot();
    if (!done[dslot]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap);
        if (e != hipSuccess) {
            aurppo_set_error("hipFuncSetAttribute(%s, hipFuncAttributeMaxDynamicSharedMemorySize, %d) failed: %s", name, (int)lds_cap,
                             hipGetErrorString(e));
            return AURPPO_EHIP;
        }
        done[dslot] = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, s, a);
    AURPPO_LAUNCH_CHECK(name);
    return AURPPO_OK;
}
// CUs of the calling thread's current device (asked once per device; `fallback` if the runtime reports none), or a negative AURPPO_E*
// code with the error set (api.hip)
int aurppo_cu_count(int fallback);
// The prepared-operand half of the linear products (linear.hip), for the layered steps (layered.hip): bytes of one forward operand
// copy of a (N, K) weight, the launch that writes it (conv.hip; mode 0; 1: the input gradient's), and y (M, N) = act(x (M, K) . w^T + bias)
// from such copies (act: 0 none, 1 tanh): `nets` same-shaped products, one operand set each, in one launch -- on k_linear's tile
// (nets = 1), or with `small` on the small-M tile (k_linear_small; nets = 2: k_linear_pair).  Same bits on either tile.  Refusals carry
// the calling entry's name `who`.
constexpr int kLayeredMaxLayers = 16;
size_t aurppo_linear_wop_bytes(int K, int N);
int linear_prep(const float* w, int K_w, int N_w, int mode, unsigned short* wop, hipStream_t s);
struct LinOps {
    const float* x;                  // (M, K)
    const void* wop;                 // the operand copy of the (N, K) weight
    const float* bias;               // (N,) or nullptr
    float* y;                        // (M, N)
};
int aurppo_linear_forward(const char* who, bool small, int nets, const LinOps* ops, int act, long long M, int K, int N, void* stream,
                          int n_bias = 0);
// The layered steps at a hidden width `hidden` that is no multiple of 32 run as the policy of width Hp = layered_padded(hidden) whose
// extra weights and biases are zero (layered.hip says why that is exact).  Where the padded shape meets the unpadded bucket:
//   linear_prep_pad (conv.hip): the operand copy of a Kg x Ng product from a smaller (N_w, K_w) weight, zero planes outside it.
//   n_bias (aurppo_linear_forward; 0: N): the bias has n_bias floats and the columns from there on add 0 -- bias[n_bias ...] is the
//     bucket's next parameter.
//   linear_product / linear_wgrad_product (linear.hip): the products behind aurppo_linear_*_f32 with the product's own dimensions
//     apart from the weight's -- Kg x Ng where the weight is (N_w, K_w) and the bias N_w floats, and (N, K) planes whose (Nr, Kr)
//     corner is the bucket's dw (db: the Nr bias gradients).  Equal dimensions: the entries' own path.
//   head_ppo_run / head_act_launch (head.hip): K13 / K14 on (rows, H) planes with head rows of Hr <= H floats in the bucket.
inline int layered_padded(int hidden) { return (hidden + 31) / 32 * 32; }
int linear_prep_pad(const float* w, int K_w, int N_w, int mode, int Kg, int Ng, unsigned short* wop, hipStream_t s);
int linear_product(const float* x, const float* w, const float* bias, int act, float* y, long long M, int K_w, int N_w, int mode, int Kg,
                   int Ng, void* wop_ws, void* stream, const int32_t* rows, const float* h);
int linear_wgrad_product(const float* dy, const float* x, const int32_t* rows, float* dw, float* db, long long M, int N, int K, int Nr, int Kr,
                         void* ws, void* stream);
int fold_slices_pad_launch(const float* part, int S, int Np, int Kp, int Nr, int Kr, float* out, const double* bpart, float* db, hipStream_t s);
// K13 / K14's shape rule (H a multiple of 32) and the two kernels on checked operands (head.hip), for the layered steps
bool head_shape_ok(int H, int A, int continuous);
// ... with at most max_a actions: 16 (head_shape_ok), or 32 for the wide-action (`wa`) entries, whose A in 17 .. 32 runs the kernels' NA = 32 builds
bool head_shape_ok_upto(int H, int A, int continuous, int max_a);
int head_ppo_run(const char* who, const float* hA, const float* hC, float* gzA, float* gzC, const float* actions, const float* rec,
                 const int32_t* idx, int M, int H, int Hr, int A, int continuous, const float* params, const int* layout_h, int n_params,
                 float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace,
                 void* stream, int max_a);
int head_act_launch(const float* hA, const float* hC, const float* noise, int N, int H, int Hr, int A, int continuous, const float* params,
                    const int* lay, float* actions, float* logp, float* value, hipStream_t s);
// The kernels conv.hip and linear.hip both run live in conv.hip: linear_prep above (k_conv_prep / k_linear_prep_tail), the fold of a
// weight gradient's S slices (db != nullptr: k_fold_slices_bias, with the column sums bpart (S, N) -> db), and the slice count.
int fold_slices_launch(const float* part, int S, long long n, float* out, const double* bpart, int N, float* db, hipStream_t s);
int slices_for(long long tiles, long long most);
// Diagnostic knobs.  Every environment variable the library looks at is parsed in ONE place (api.hip) into this struct,
// once per process -- or on every call when AURPPO_TEST_KNOBS=1 (tests/conftest.py), so that one test process can flip
// them.  None of them changes results beyond summation order; the defaults are the product configuration.
struct AurppoKnobs {
    int k7_variant;        // AURPPO_K7_VARIANT: 3 (default) = 3 x bf16-split MFMA k_mlp_step3 (mlp3.hip), 2 = f32 MFMA k_mlp_step2; always one of the two (api.hip normalises)
    int k7w_variant;       // AURPPO_K7W_VARIANT: 3 (default) = k_mlpw3_step (bf16x3 MFMA) for the shapes wider than 64, 2 = the fp32-MFMA k_mlpw_step
    int k7_spare_cus;      // AURPPO_MLP_SPARE_CUS: CUs K7 / K7w leave to the side stream's shuffle kernels (default 8)
    int static_tiles;      // AURPPO_STATIC_TILES=1: K7 / K7w deal tiles by static stride instead of through the counter, which
                           // fixes the order of every sum (bit-reproducible gradients; tests/test_determinism.py)
    int k2_one_stream;     // AURPPO_K2_ONE_STREAM=1: the twist on the caller's stream (serial with the accepts; link + resolve keep their own)
    int k2_link_wgs;       // AURPPO_K2_LINK_WGS: workgroups of k_fy_link (default 48; 0 = one per 256 positions)
    int k2_resolve_wgs;    // AURPPO_K2_RESOLVE_WGS: workgroups of k_fy_resolve (default 256; 0 = one per 256 positions)
    int k2_starve;         // AURPPO_TEST_K2_STARVE (tests): the twist keeps this per cent of one shuffle's draws in stock, so shuffles run dry
    int k2_accept3_wgs;    // AURPPO_K2_ACCEPT3_WGS: workgroups of k_fy_accept3's relay (default 6)
    int gather_unroll;     // AURPPO_GATHER_UNROLL (0 = by row width)
    int gather_rows;       // AURPPO_GATHER_ROWS (0 = by row width)
};
const AurppoKnobs& aurppo_knobs();

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// Sum over a workgroup of NW waves; result valid in thread 0.  `scratch` holds NW doubles per
// concurrent value; callers separate uses with __syncthreads().
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < NW; ++w) r += scratch[w];
    }
    return r;
}

static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
