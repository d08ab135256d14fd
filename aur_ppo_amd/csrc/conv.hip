// K11 -- 3x3 convolution (stride 1, zero padding 0..2) as an implicit GEMM on the bf16 matrix pipe: the hidden blocks of the
// robot policy's encoder (src/nets/base_cnns.py:32-45: nn.Conv2d(16,32,3,padding=1) ... nn.Conv2d(256,256,3)), forward AND the
// gradient with respect to the input (the same product with the filter transposed and flipped, padding 2 - p).
//
// Why: rocprofv3 counters over robot_ppo.update (profiles/r04/robot5_mfma_pmc.json) show the library's choice for these layers,
// miopenSp3AsmConv_v30_3_1_gfx9_fp32_f2x3 (Winograd F(2,3), 36-46 % of the update), issuing NO matrix instruction -- it is
// vector-ALU code, bounded by the 157 TFLOP/s fp32 FMA rate (x 2.25 for Winograd's fewer multiplies); fp32 products formed
// as six bf16 MFMAs (bf16x3.h, fp32-equivalent) have a ceiling of 2 500 / 6 = 417 TFLOP/s.
//
// GEMM view: M = output pixels of the whole batch, flattened (b, y, x); N = output channels; K = (tap, input channel), 16
// consecutive input channels of one tap per k-step (every hidden layer's width is a multiple of 16).  A wave owns 32
// consecutive pixels x up to four 32-channel blocks (4 x 16 accumulator registers):
//   * A operand straight from global memory, no LDS staging: lane (pixel m, half h) loads its 8 channels of the tap's input pixel
//     (NCHW: 8 dword loads, coalesced across the 32 pixels of the wave; zero outside the image), splits them into three bf16
//     planes in registers (44 vector instructions per k-step, against 6 x NB matrix instructions) -- a pixel is re-read once
//     per tap and channel group, from L1 / L2; the k-step after the current one is in flight while it computes;
//   * B operand: the filter as bf16 planes in operand order (k_conv_prep, L2-resident; the four waves of a workgroup work on
//     neighbouring pixel blocks of the same channel group and share its lines in L1);
//   * epilogue: the 32 x 32 accumulator blocks go through a padded LDS tile so that the stores are 128-byte rows of an output
//     plane instead of 16-byte pieces of 64 planes.
// Output is the convolution without bias (the block's bias + ReLU + max-pool tail is K9, csrc/pool.hip) -- or, in the POOL builds
// (K11p, aurppo_conv3x3_pool_f32), the whole block's pooled output and K9's mask, that tail taken in the epilogue.
#pragma clang fp contract(fast)
#include "bf3_gemm.h"
#include "common.h"

using namespace bf3;

namespace {

struct ConvArgs {
    const float* x;                  // (B, Cin, H, W)
    const unsigned short* wop;       // [n-block][k-step = tap * CG + cg][plane][lane][8]
    float* z;                        // (B, Cout, Ho, Wo)
    int B, Cin, H, W, Cout, Ho, Wo, pad;
    long long M;                     // B * Ho * Wo
    int CG;                          // Cin / 16
    int n_mb4;                       // workgroups along M (4 waves x kMB pixel blocks each)
};

// K11p (the POOL builds): the same product whose epilogue adds the bias and takes ReLU + the 2 x 2 max-pool of K9 (csrc/pool.hip), so
// the full-resolution pre-activation is never stored.
struct ConvPoolArgs {
    ConvArgs c;                      // the product, with Ho x Wo the POOLED map ((H + 2 pad - 2) >> 1, ...), z (B, Cout, Ho, Wo) the
                                     // block's pooled output and M = 4 * B * Ho * Wo, the four positions of every window
    const float* bias;               // (Cout,) or nullptr
    uint8_t* mask;                   // (B, Cout, Ho, Wo): K9's byte
};

// K11x (the XPL / OPL builds): activations as bf16 planes, uint16 [b][c / 8][plane][pixel][8] (include/aurppo.h)
struct ConvPlanesArgs {
    ConvPoolArgs p;                  // (without POOL: p.c alone)
    const unsigned short* xp;        // XPL: the input's planes (p.c.x is not read)
    unsigned short* yp;              // OPL: the pooled output's planes, beside p.c.z and p.mask
};

// One pixel block's A values of a k-step in an XPL build are its three planes, in an fp32 build eight floats: the body's text names
// both, and only the including build's kind is ever called.
__device__ __forceinline__ void put_plane(u32x4 (&d)[3], int pl, u32x4 t) { d[pl] = t; }
[[maybe_unused]] __device__ __forceinline__ void put_plane(float (&)[8], int, u32x4) {}
__device__ __forceinline__ u32x4 get_plane(const u32x4 (&d)[3], int pl) { return d[pl]; }
[[maybe_unused]] __device__ __forceinline__ u32x4 get_plane(const float (&)[8], int) { return u32x4{0u, 0u, 0u, 0u}; }

// filter -> operand order.  transpose_flip = 0 (forward): B[k = (tap, ci)][n = co] = W[co][ci][tap];
// 1 (input gradient): the product's "input" channels are the forward pass's OUTPUT channels: B[k = (tap, co)][n = ci] =
// W[co][ci][8 - tap].  cin_gemm / cout_gemm are the product's own channel counts (cin_gemm a multiple of 16).
// KTAIL (k_linear_prep_tail: a linear layer whose inner dimension Ci_w is no multiple of 16, forward only): cin_gemm is Ci_w rounded
// up to whole k-steps, and the columns k >= Ci_w -- which w does not have -- get zero planes without a read.
template <bool KTAIL>
__device__ __forceinline__ void conv_prep_body(const float* __restrict__ w, int Co_w, int Ci_w, int cin_gemm, int cout_gemm,
                                               int transpose_flip, unsigned short* __restrict__ wop, int taps) {
    const int CG = cin_gemm >> 4, KS = taps * CG, NBLK = (cout_gemm + 31) >> 5;
    const long long total = (long long)NBLK * KS * 64 * 8;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        const long long r = e >> 9;
        const int ks = (int)(r % KS), nblk = (int)(r / KS);
        const int tap = ks / CG, cg = ks - tap * CG;
        const int n = nblk * 32 + (lane & 31), k = cg * 16 + 8 * (lane >> 5) + j;
        float v = 0.0f;
        if (n < cout_gemm && (!KTAIL || k < Ci_w)) {
            if (!transpose_flip) v = w[((size_t)n * Ci_w + k) * taps + tap];               // W[co = n][ci = k][tap]
            else v = w[((size_t)k * Ci_w + n) * taps + (taps - 1 - tap)];                  // W[co = k][ci = n][flipped tap]
        }
        unsigned p0, p1, p2;
        split3(v, 0.0f, p0, p1, p2);
        const size_t at = (((size_t)(nblk * KS + ks) * 3) * 64 + lane) * 8 + j;
        wop[at] = (unsigned short)p0;
        wop[at + 512] = (unsigned short)p1;
        wop[at + 1024] = (unsigned short)p2;
    }
    (void)Co_w;
}
__global__ __launch_bounds__(256) void k_conv_prep(const float* __restrict__ w, int Co_w, int Ci_w, int cin_gemm, int cout_gemm,
                                                   int transpose_flip, unsigned short* __restrict__ wop, int taps) {
    conv_prep_body<false>(w, Co_w, Ci_w, cin_gemm, cout_gemm, transpose_flip, wop, taps);
}
__global__ __launch_bounds__(256) void k_linear_prep_tail(const float* __restrict__ w, int N_w, int K_w, int k_gemm,
                                                          unsigned short* __restrict__ wop) {
    conv_prep_body<true>(w, N_w, K_w, k_gemm, N_w, 0, wop, 1);
}

// k_linear_prep_pad: the operand copy of a linear product that runs wider than its weight -- the layered steps at a hidden width
// that is no multiple of 32 (layered.hip), whose products from layer 1 on run at Hp = the width rounded up.  The product is
// k_gemm (whole k-steps) x n_gemm; the weight is (N_w, K_w) and ends where it ends -- behind the bucket's last matrix there is nothing
// -- so an element is read only where BOTH its indices lie inside the weight, and every other one is a zero plane: mode 0 the
// columns n >= N_w and the k-rows >= K_w, mode 1 (B[k = n_w][n = k_w]) the k-rows >= N_w and the columns >= K_w.
__global__ __launch_bounds__(256) void k_linear_prep_pad(const float* __restrict__ w, int N_w, int K_w, int mode, int k_gemm, int n_gemm,
                                                         unsigned short* __restrict__ wop) {
    const int KS = k_gemm >> 4, NBLK = (n_gemm + 31) >> 5;
    const long long total = (long long)NBLK * KS * 64 * 8;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        const long long r = e >> 9;
        const int ks = (int)(r % KS), nblk = (int)(r / KS);
        const int n = nblk * 32 + (lane & 31), k = ks * 16 + 8 * (lane >> 5) + j;
        float v = 0.0f;
        if (mode == 0) {
            if (n < N_w && k < K_w) v = w[(size_t)n * K_w + k];
        } else if (k < N_w && n < K_w) v = w[(size_t)k * K_w + n];
        unsigned p0, p1, p2;
        split3(v, 0.0f, p0, p1, p2);
        const size_t at = (((size_t)(nblk * KS + ks) * 3) * 64 + lane) * 8 + j;
        wop[at] = (unsigned short)p0;
        wop[at + 512] = (unsigned short)p1;
        wop[at + 1024] = (unsigned short)p2;
    }
}

// Workgroup = 4 waves x (2 x 32 pixels) = 256 consecutive output pixels x NB 32-channel blocks.  The filter's fragments of two
// k-steps at a time (kKC x NB x 3 KB) are brought into LDS ONCE per workgroup by LDS-DMA, double-buffered, one barrier per chunk;
// every wave reads its B fragments from there (with each wave fetching its own from L2, the CU's L2 path -- about 16 B per
// cycle -- carried 12 KB per wave and k-step: 61-120 TFLOP/s, no better than the library).
// BUF (the input tensor is under 4 GB): the A values come through buffer loads -- per lane ONE 32-bit byte offset per tap and
// pixel block (out-of-image taps get an offset past the buffer: the hardware returns 0), the channel's offset in a scalar
// register.  The first version formed a 64-bit address and a zero select per value: 288 vector instructions per k-step against
// 48 matrix instructions, and the two barely overlap (SQ_VALU_MFMA_COEXEC_CYCLES 7 % of the matrix time, profiles/r04).
template <int NB, bool BUF>      // NB: 32-channel blocks of the channel group (1, 2 or 4)
__global__ __launch_bounds__(kConvThreads, 2) void k_conv3x3(const ConvArgs a) {
    constexpr bool POOL = false, XPL = false, OPL = false;
    constexpr const float* pool_bias = nullptr;
    constexpr uint8_t* pool_mask = nullptr;
    constexpr const unsigned short* in_planes = nullptr;
    constexpr unsigned short* out_planes = nullptr;
#include "conv3x3_body.h"
}
// The POOL builds (K11p, conv3x3_body.h says what they are) are an overload with a third template parameter and their own argument
// block, not a defaulted parameter on the template above: that one keeps its symbols and its instruction streams.
template <int NB, bool BUF, bool POOL>
__global__ __launch_bounds__(kConvThreads, 2) void k_conv3x3(const ConvPoolArgs p) {
    static_assert(POOL, "the plain builds are k_conv3x3<NB, BUF>");
    const ConvArgs& a = p.c;
    constexpr bool XPL = false, OPL = false;
    const float* const pool_bias = p.bias;
    uint8_t* const pool_mask = p.mask;
    constexpr const unsigned short* in_planes = nullptr;
    constexpr unsigned short* out_planes = nullptr;
#include "conv3x3_body.h"
}
// K11x (the XPL / OPL builds, conv3x3_body.h says what they are): again an overload with its own argument block, forward products only.
// XPL without POOL is K11 on planes (q.p.c alone, with c.x unused); with POOL it is K11p reading planes, writing them (OPL), or both.
template <int NB, bool BUF, bool POOL, bool XPL, bool OPL>
__global__ __launch_bounds__(kConvThreads, 2) void k_conv3x3(const ConvPlanesArgs q) {
    static_assert(XPL || OPL, "the fp32 builds are k_conv3x3<NB, BUF> and k_conv3x3<NB, BUF, true>");
    static_assert(POOL || !OPL, "planes are written by the pooled epilogue");
    const ConvArgs& a = q.p.c;
    [[maybe_unused]] const float* const pool_bias = q.p.bias;
    [[maybe_unused]] uint8_t* const pool_mask = q.p.mask;
    [[maybe_unused]] const unsigned short* const in_planes = q.xp;
    [[maybe_unused]] unsigned short* const out_planes = q.yp;
#include "conv3x3_body.h"
}

// fp32 NCHW -> planes (include/aurppo.h: uint16 [b][c / 8][plane][pixel][8]): a thread takes one pixel of one group of eight channels --
// eight dword loads, coalesced over the pixels, and one 16-byte store per plane.  The DEFINITION of the layout: what an OPL producer
// writes and what an XPL build reads is what this kernel leaves.
__global__ __launch_bounds__(256) void k_split_planes(const float* __restrict__ x, unsigned short* __restrict__ xp, long long n_groups,
                                                      int HW) {
    const long long total = n_groups * HW;        // n_groups = B * C / 8
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long bg = e / HW;
        const int px = (int)(e - bg * HW);
        const float* const src = x + (size_t)bg * 8 * HW + px;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(size_t)j * HW];
        unsigned p[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) split3(v[2 * q], v[2 * q + 1], p[q][0], p[q][1], p[q][2]);
        u32x4* const dst = reinterpret_cast<u32x4*>(xp) + (size_t)bg * 3 * HW + px;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) dst[(size_t)pl * HW] = u32x4{p[0][pl], p[1][pl], p[2][pl], p[3][pl]};
    }
}

// ---- K12: the 3x3 convolution's WEIGHT gradient on the same arithmetic.
//     dW[co][ci][ky][kx] = sum over (b, y, x) of dY[b][co][y][x] * X[b][ci][y + ky - p][x + kx - p]
// as a product C[m = co][n = ci * 9 + tap] = A[m][k = pixel] . B[k = pixel][n] whose inner dimension is the batch's output pixels
// (flattened) and whose output IS the filter's memory layout.  Both operands are new every k-step, so both are split: once per
// WORKGROUP, through LDS.  In NCHW the inner dimension is the contiguous one of both operands (a channel's pixels), which is the
// F image of bf16x3.h ([row = channel][32 samples], 8-byte stores of 4 consecutive samples, fragments by ds_read_b128 along a
// row): one image holds the workgroup's dY channels (64 WM rows) and its (ci, tap) columns (64 (4 / WM) rows) for a chunk of
// 32 pixels; each of the four waves forms a 64 x 64 part (2 x 2 accumulator blocks) of the tile.
//   * a thread stages 4 consecutive pixels of 8 (10) rows; the pixels' offsets / tap masks of a chunk come from a 32-entry table
//     that 32 lanes fill ahead of its use (two integer divisions per pixel, once per workgroup instead of once per row);
//   * loads are buffer loads relative to the slice's first image (32-bit offsets whatever the tensor's size); a tap outside the
//     image, a row past the tensor and a pixel past the slice get an offset past the buffer: the hardware returns 0.  QUAD (the
//     map's width a multiple of 4, padding <= 1: a quad of output pixels never leaves its row): one 16-byte load per row and
//     quad -- the X quad of a tap one column to the left starts at its second pixel and is shifted in registers;
//   * the values of chunk c + 2 are requested while chunk c is multiplied (two register sets);
//   * the pixels are cut into S slices (grid = tiles x S); k_fold_slices sums the partial filters in slice order (deterministic).
struct ConvWgradArgs {
    const float* dy;                 // (B, Co, Ho, Wo)
    const float* x;                  // (B, Ci, H, W)
    float* part;                     // (S, Co, Ci * 9)
    int B, Ci, H, W, Co, Ho, Wo, pad;
    long long M;                     // B * Ho * Wo
    int NK;                          // Ci * 9
    int px_per_slice;                // a multiple of 32
    int n_tiles_m, n_tiles_n;
};

constexpr unsigned kOob = 0x80000000u;      // buffer offsets from here on read 0 (num_records <= 2^31)

template <int PL>
__device__ __forceinline__ Frag3 wg_rows(const char* img, int f0, int ks, int lane) {       // A[m = f0 + ..][k] / B[k][n = f0 + ..]
    const int o = (foff(lane & 31, 8 * (lane >> 5)) ^ (ks << 5)) + f0 * kFRow;      // (f0 a multiple of 16: lane part + constants, bf16x3.h)
    Frag3 f;
#pragma unroll
    for (int p = 0; p < 3; ++p) f.p[p] = lds_b128(img + p * PL + o);
    return f;
}

template <int WM, bool QUAD>      // WM waves along the output channels: tile = 64 WM channels x 64 (4 / WM) filter columns
__global__ __launch_bounds__(kConvThreads, 2) void k_conv3x3_wgrad(const ConvWgradArgs a) {
    constexpr int kRowsA = 64 * WM, kRowsB = 64 * (4 / WM), kSlotsA = 2 * WM, kSlots = (kRowsA + kRowsB) / 32;
    constexpr int PL = (kRowsA + kRowsB) * kFRow;         // one bf16 plane of the image
    __shared__ __attribute__((aligned(16))) char s_img[3 * PL];
    // per chunk (three in flight): row 0 = the dY offsets of its 32 pixels, rows 1..9 = the X offsets per tap (the tap's shift
    // included); a pixel past the slice / a tap outside the image holds kOob
    __shared__ __attribute__((aligned(16))) unsigned s_tab[3][10][32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = a.n_tiles_m * a.n_tiles_n;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), s = (int)(blockIdx.x / (unsigned)tiles);
    const int co0 = (tile / a.n_tiles_n) * kRowsA, n0 = (tile % a.n_tiles_n) * kRowsB;
    const int HoWo = a.Ho * a.Wo, HW = a.H * a.W;
    const long long m_lo = (long long)s * a.px_per_slice;
    long long m_hi = m_lo + a.px_per_slice;
    if (m_hi > a.M) m_hi = a.M;
    const int n_px = (int)(m_hi - m_lo);
    const int b_lo = (int)(m_lo / HoWo), r_lo = (int)(m_lo - (long long)b_lo * HoWo);
    // buffers that start at the slice's first image
    const size_t left_a = (size_t)(a.B - b_lo) * a.Co * HoWo * 4, left_b = (size_t)(a.B - b_lo) * a.Ci * HW * 4;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy + (size_t)b_lo * a.Co * HoWo), 0, (unsigned)(left_a < kOob ? left_a : kOob), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x + (size_t)b_lo * a.Ci * HW), 0, (unsigned)(left_b < kOob ? left_b : kOob), 0x00020000);
    // this thread's image rows (crow + 32 u) and its pixel quad
    const int q4 = (tid & 7) * 4, crow = tid >> 3;
    // rows past the tensor (channels >= Co, filter columns >= Ci * 9) are staged from wherever offset 0 + ... lands or from beyond
    // the buffer: their products are never stored
    unsigned row_off[kSlots];
    int row_tap[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
        const int row = crow + 32 * u;
        if (u < kSlotsA) {
            const int co = co0 + row;
            row_off[u] = co < a.Co ? (unsigned)co * (unsigned)HoWo * 4u : kOob;
            row_tap[u] = 0;
        } else {
            const int n = n0 + row - kRowsA;
            const int ci = n / 9;
            row_off[u] = n < a.NK ? (unsigned)(ci * HW) * 4u : kOob;
            row_tap[u] = 1 + (n - 9 * ci);
        }
    }
    // The table of chunk c: lane i < 32 of EVERY wave decomposes pixel i (two divisions by float reciprocal + fix-up: the slice's
    // pixel indices stay below 2^23, conv_wgrad_plan) and wave w fills rows w, w + 4, w + 8 -- left to 32 lanes of one wave, the
    // nine taps and two integer divisions were ~190 vector instructions per chunk on the wave every barrier waits for.
    const float inv_howo = 1.0f / (float)HoWo, inv_wo = 1.0f / (float)a.Wo;
    auto fdiv = [](int n, int d, float inv, int& rem) {
        int q = (int)((float)n * inv);
        int r = n - q * d;
        if (r < 0) { q -= 1; r += d; }
        else if (r >= d) { q += 1; r -= d; }
        rem = r;
        return q;
    };
    auto table = [&](int c) {
        if (lane < 32) {
            const int i = c * 32 + lane;
            unsigned (*const tab)[32] = s_tab[c % 3];
            int r, x;
            const int b = fdiv(r_lo + i, HoWo, inv_howo, r);        // (relative to the first pixel of image b_lo)
            const int y = fdiv(r, a.Wo, inv_wo, x);
            const int base = b * a.Ci * HW + (y - a.pad) * a.W + (x - a.pad);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int t = w + 4 * k;                             // (wave-uniform)
                if (t < 10) {
                    unsigned e;
                    if (t == 0) {
                        e = (unsigned)(b * a.Co * HoWo + r) * 4u;
                    } else {
                        const int ky = (t - 1) / 3, kx = (t - 1) - 3 * ky;
                        const int iy = y + ky - a.pad, ix = x + kx - a.pad;
                        const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                        e = in ? (unsigned)(base + ky * a.W + kx) * 4u : kOob;
                    }
                    tab[t][lane] = i < n_px ? e : kOob;
                }
            }
        }
    };
    // (the loads' results are not touched here: the shift of a row-start quad and the zero of a row-end pixel wait in `fl` -- two bits
    // per row -- until the chunk is split, two chunks later.  Applied at this point, the selects sat right behind the loads and every
    // request was a wait for its own loads.)
    auto fetch = [&](int c, float (&v)[kSlots][4], unsigned& fl) {
        const unsigned (*const tab)[32] = s_tab[c % 3];
        fl = 0u;
#pragma unroll
        for (int u = 0; u < kSlots; ++u) {
            const u32x4 t = *reinterpret_cast<const u32x4*>(&tab[row_tap[u]][q4]);        // this row's offsets of the quad's pixels
            if (QUAD) {
                // the quad sits in one row of its image: pixel 1 is inside the image for every tap whose row is (W >= 4, pad <= 1);
                // pixel 0 / pixel 3 may fall off the row's ends
                u32x4 L;
                if (u < kSlotsA) {
                    L = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, t.x + row_off[u], 0, 0));
                    v[u][0] = __uint_as_float(L.x); v[u][1] = __uint_as_float(L.y);
                    v[u][2] = __uint_as_float(L.z); v[u][3] = __uint_as_float(L.w);
                } else {
                    const bool shl = t.x >= kOob;                 // pixel 0 is off the row: the load starts at pixel 1
                    const unsigned off = t.y < kOob ? (shl ? t.y : t.y - 4u) : kOob;
                    L = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, off + row_off[u], 0, 0));
                    v[u][0] = __uint_as_float(L.x); v[u][1] = __uint_as_float(L.y);
                    v[u][2] = __uint_as_float(L.z); v[u][3] = __uint_as_float(L.w);
                    fl |= (shl ? 1u : 0u) << (2 * u);
                    fl |= (t.w < kOob ? 0u : 2u) << (2 * u);
                }
            } else {
                const __amdgpu_buffer_rsrc_t r = u < kSlotsA ? ra : rb;
                v[u][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.x + row_off[u], 0, 0));
                v[u][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.y + row_off[u], 0, 0));
                v[u][2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.z + row_off[u], 0, 0));
                v[u][3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.w + row_off[u], 0, 0));
            }
        }
    };
    const int wn = WM == 2 ? (w >> 1) : 0, wk = WM == 2 ? (w & 1) : w;
    const int rowA = wn * 64, rowB = kRowsA + wk * 64;
    f32x16c acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int n_chunks = (n_px + 31) >> 5;
    // one chunk: its values (requested two chunks ago) -> planes -> products; meanwhile chunk c + 2 is requested into the same registers
    auto step = [&](int c, float (&v)[kSlots][4], unsigned& fl) {
        __syncthreads();                                    // the previous chunk's fragments have been read; table c + 2 is written
#pragma unroll
        for (int u = 0; u < kSlots; ++u) {
            float x0 = v[u][0], x1 = v[u][1], x2 = v[u][2], x3 = v[u][3];
            if (QUAD && u >= kSlotsA) {
                const bool shl = (fl >> (2 * u)) & 1u, z3 = (fl >> (2 * u + 1)) & 1u;
                x3 = shl ? x2 : (z3 ? 0.0f : x3);
                x2 = shl ? x1 : x2;
                x1 = shl ? x0 : x1;
                x0 = shl ? 0.0f : x0;
            }
            unsigned a0, a1, a2, b0, b1, b2;
            split3(x0, x1, a0, a1, a2);
            split3(x2, x3, b0, b1, b2);
            const int o = foff(crow, q4) + 32 * u * kFRow;      // = foff(crow + 32 u, q4)
            *reinterpret_cast<u32x2*>(s_img + 0 * PL + o) = u32x2{a0, b0};
            *reinterpret_cast<u32x2*>(s_img + 1 * PL + o) = u32x2{a1, b1};
            *reinterpret_cast<u32x2*>(s_img + 2 * PL + o) = u32x2{a2, b2};
        }
        __syncthreads();
        if (c + 2 < n_chunks) fetch(c + 2, v, fl);
        if (c + 3 < n_chunks) table(c + 3);                 // (slot c % 3: last read by fetch(c), before this chunk's first barrier)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            Frag3 A0 = wg_rows<PL>(s_img, rowA, ks, lane), A1 = wg_rows<PL>(s_img, rowA + 32, ks, lane);
            const Frag3 B0 = wg_rows<PL>(s_img, rowB, ks, lane), B1 = wg_rows<PL>(s_img, rowB + 32, ks, lane);
            if (kStepNeg(ks)) {                              // (ks is a constant of the unrolled loop)
                A0 = neg3(A0); A1 = neg3(A1);
                acc[0][0] = mma32x3_step<true>(A0, B0, acc[0][0]);
                acc[0][1] = mma32x3_step<true>(A0, B1, acc[0][1]);
                acc[1][0] = mma32x3_step<true>(A1, B0, acc[1][0]);
                acc[1][1] = mma32x3_step<true>(A1, B1, acc[1][1]);
            } else {
                acc[0][0] = mma32x3_step<false>(A0, B0, acc[0][0]);
                acc[0][1] = mma32x3_step<false>(A0, B1, acc[0][1]);
                acc[1][0] = mma32x3_step<false>(A1, B0, acc[1][0]);
                acc[1][1] = mma32x3_step<false>(A1, B1, acc[1][1]);
            }
        }
    };
    float va[kSlots][4], vb[kSlots][4];
    unsigned fa = 0u, fb = 0u;
    table(0);
    if (n_chunks > 1) table(1);
    if (n_chunks > 2) table(2);
    __syncthreads();
    fetch(0, va, fa);
    if (n_chunks > 1) fetch(1, vb, fb);
    for (int c = 0; c < n_chunks; c += 2) {
        step(c, va, fa);
        if (c + 1 < n_chunks) step(c + 1, vb, fb);
    }
    // C[m = co][n]: the lane holds the filter column, its registers the channels -- rows of `part` are contiguous over the lanes
    float* const out = a.part + (size_t)s * a.Co * a.NK;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wk * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = co0 + rowA + i * 32 + acc_row_c(e, lane);
                if (row < a.Co && col < a.NK) out[(size_t)row * a.NK + col] = acc[i][j][e];
            }
        }
}

// part[0][i] + part[1][i] + ... in slice order
__device__ __forceinline__ float fold_slices_at(const float* __restrict__ part, int S, long long n, long long i) {
    float t = 0.0f;
    int sl = 0;
    for (; sl + 8 <= S; sl += 8) {
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = part[(size_t)(sl + k) * n + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) t += x[k];
    }
    for (; sl < S; ++sl) t += part[(size_t)sl * n + i];
    return t;
}
__global__ __launch_bounds__(256) void k_fold_slices(const float* __restrict__ part, int S, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = fold_slices_at(part, S, n, i);
}
// k_fold_slices with the BIAS builds' partial column sums behind it: the workgroups past the last of the fold add bpart (S, N) in
// slice order, still in fp64, and round once into db (N,).
__global__ __launch_bounds__(256) void k_fold_slices_bias(const float* __restrict__ part, int S, long long n, float* __restrict__ out,
                                                          const double* __restrict__ bpart, int N, float* __restrict__ db) {
    const long long n_fold = (n + 255) / 256;
    if ((long long)blockIdx.x >= n_fold) {
        const long long j = ((long long)blockIdx.x - n_fold) * 256 + threadIdx.x;
        if (j >= N) return;
        double t = 0.0;
        for (int sl = 0; sl < S; ++sl) t += bpart[(size_t)sl * N + j];
        db[j] = (float)t;
        return;
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = fold_slices_at(part, S, n, i);
}

// The fold of a weight gradient that ran on padded planes (the layered steps at a hidden width that is no multiple of 32): the slices
// are (Np, Kp) -- n_p floats apart -- and out is the bucket's (Nr, Kr) matrix at its own row stride, so thread i = (r, c) of Nr x Kr
// sums element r * Kp + c of every slice, in k_fold_slices' order, and nothing is written for a pad row or column.  The workgroups
// past the last of the fold add the BIAS builds' bpart (S, Np) for the Nr real columns only (launched where db != nullptr).
__global__ __launch_bounds__(256) void k_fold_slices_pad(const float* __restrict__ part, int S, long long n_p, int Kp, int Nr, int Kr,
                                                         float* __restrict__ out, const double* __restrict__ bpart, int Np,
                                                         float* __restrict__ db) {
    const long long n = (long long)Nr * Kr, n_fold = (n + 255) / 256;
    if ((long long)blockIdx.x >= n_fold) {
        const long long j = ((long long)blockIdx.x - n_fold) * 256 + threadIdx.x;
        if (j >= Nr) return;
        double t = 0.0;
        for (int sl = 0; sl < S; ++sl) t += bpart[(size_t)sl * Np + j];
        db[j] = (float)t;
        return;
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long r = i / Kr;
    out[i] = fold_slices_at(part, S, n_p, r * Kp + (i - r * Kr));
}

// The host side of K11's four forward entries (first_block_fwd of pool.hip is the model): every refusal under the entry's name `who`, then
// the argument block, the grid and the build, the filter's operand copy (k_conv_prep of the (Co_w, Ci_w, 3, 3) filter, transposed and
// flipped for an input gradient) and the product -- every refusal before the first launch.  cin / cout / p are the product's own (the
// entry has mapped its mode).  `pool`: K11p -- z and mask hold the pooled map, the product's rows are the four positions of each of its
// windows.  `planes`: a K11x entry -- xp (the input as planes, x then null) and / or yp (the pooled output's planes, K11p's epilogue only),
// both 16-byte aligned, yp with whole groups of eight output channels.
struct ConvPlan {
    ConvPlanesArgs q;                // (K11 launches with q.p.c alone, K11p with q.p)
    Bf3Grid g;
    bool buf;                        // the BUF builds
};
template <bool POOL, bool XPL, bool OPL>
void launch_conv(const ConvPlan& pl, hipStream_t s) {
    const dim3 g((unsigned)(pl.g.n_mb * pl.g.n_ng)), blk(kConvThreads);
    bf3_with_nb(pl.g.NB, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        if constexpr (XPL || OPL) {
            if (pl.buf) hipLaunchKernelGGL((k_conv3x3<NB, true, POOL, XPL, OPL>), g, blk, 0, s, pl.q);
            else hipLaunchKernelGGL((k_conv3x3<NB, false, POOL, XPL, OPL>), g, blk, 0, s, pl.q);
        } else if constexpr (POOL) {
            if (pl.buf) hipLaunchKernelGGL((k_conv3x3<NB, true, true>), g, blk, 0, s, pl.q.p);
            else hipLaunchKernelGGL((k_conv3x3<NB, false, true>), g, blk, 0, s, pl.q.p);
        } else {
            if (pl.buf) hipLaunchKernelGGL((k_conv3x3<NB, true>), g, blk, 0, s, pl.q.p.c);
            else hipLaunchKernelGGL((k_conv3x3<NB, false>), g, blk, 0, s, pl.q.p.c);
        }
    });
}
int conv_fwd(const char* who, bool pool, bool planes, const float* x, const unsigned short* xp, const float* w, const float* bias, float* z,
             uint8_t* mask, unsigned short* yp, void* wop_ws, int B, int cin, int cout, int H, int W, int p, int Co_w, int Ci_w,
             int transpose_flip, hipStream_t s) {
    // what K11p and K11x add to K11's pointers is looked at ahead of the padding, K11's own behind it
    AURPPO_REQUIRE((!pool || mask) && (!planes || x || xp), AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(p >= 0 && p <= 2, AURPPO_ESHAPE, "%s: pad=%d (0..2)", who, transpose_flip ? 2 - p : p);      // (the entry's own pad)
    AURPPO_REQUIRE((x || xp) && w && z && wop_ws, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(aligned_to(xp, 16) && aligned_to(yp, 16), AURPPO_EINVAL, "%s: planes not 16-byte aligned", who);
    AURPPO_REQUIRE(B > 0 && H > 0 && W > 0 && cin > 0 && cout > 0 && cin % 16 == 0, AURPPO_ESHAPE,
                   "%s: B=%d H=%d W=%d, %d input channels (a multiple of 16), %d output channels", who, B, H, W, cin, cout);
    AURPPO_REQUIRE(H + 2 * p - 2 > 0 && W + 2 * p - 2 > 0, AURPPO_ESHAPE, "%s: empty output (%d x %d)", who, H + 2 * p - 2, W + 2 * p - 2);
    AURPPO_REQUIRE((size_t)B * cin * H * W < ((size_t)1 << 40) && aligned_to(wop_ws, 16), AURPPO_ESHAPE,
                   "%s: operand too large / workspace not 16-byte aligned", who);
    AURPPO_REQUIRE(!yp || cout % 8 == 0, AURPPO_ESHAPE, "%s: %d output channels as planes (a multiple of 8)", who, cout);
    ConvPlan pl{};
    pl.q.p.bias = bias; pl.q.p.mask = mask; pl.q.xp = xp; pl.q.yp = yp;
    ConvArgs& a = pl.q.p.c;
    a.x = x; a.wop = reinterpret_cast<unsigned short*>(wop_ws); a.z = z;
    a.B = B; a.Cin = cin; a.H = H; a.W = W; a.Cout = cout; a.pad = p;
    a.Ho = H + 2 * p - 2; a.Wo = W + 2 * p - 2;
    if (pool) { a.Ho >>= 1; a.Wo >>= 1; }
    a.M = (pool ? 4ll : 1ll) * B * a.Ho * a.Wo;
    a.CG = cin / 16;
    pl.g = bf3_grid(a.M, cout);
    AURPPO_REQUIRE(pl.g.n_mb < (1ll << 30), AURPPO_ESHAPE, "%s: too many pixel blocks", who);
    a.n_mb4 = (int)pl.g.n_mb;
    AURPPO_REQUIRE(pl.g.n_mb * pl.g.n_ng < (1ll << 31), AURPPO_ESHAPE, "%s: grid too large", who);
    AURPPO_REQUIRE(!pool || (a.Ho >= 1 && a.Wo >= 1), AURPPO_ESHAPE, "%s: no whole 2 x 2 window in a %d x %d map", who, H + 2 * p - 2,
                   W + 2 * p - 2);
    // buffer loads address 32 bits: inputs under 4 GB (minus the slack a negative tap offset may wrap through); larger ones keep 64-bit addresses
    // (planes hold 6 bytes an element: the same limit, reached 1.5 x sooner)
    pl.buf = (size_t)B * cin * H * W * (xp ? 6 : 4) < ((size_t)1 << 32) - ((size_t)1 << 20);
    hipLaunchKernelGGL(k_conv_prep, dim3(128), dim3(256), 0, s, w, Co_w, Ci_w, cin, cout, transpose_flip, reinterpret_cast<unsigned short*>(wop_ws), 9);
    AURPPO_LAUNCH_CHECK("k_conv_prep");
    if (!planes) {
        if (!pool) launch_conv<false, false, false>(pl, s);
        else launch_conv<true, false, false>(pl, s);
        AURPPO_LAUNCH_CHECK(pool ? "k_conv3x3 (pool)" : "k_conv3x3");
    } else {
        if (!pool) launch_conv<false, true, false>(pl, s);
        else if (xp && yp) launch_conv<true, true, true>(pl, s);
        else if (xp) launch_conv<true, true, false>(pl, s);
        else launch_conv<true, false, true>(pl, s);
        AURPPO_LAUNCH_CHECK(pool ? "k_conv3x3 (pool, planes)" : "k_conv3x3 (planes)");
    }
    return AURPPO_OK;
}

}  // namespace

// ---- the kernels linear.hip runs too, as host functions (common.h).  linear_prep: the operand copy of a linear product's (N_w, K_w)
// weight (forward B[k][n] = w[n][k]; input gradient B[k = n_w][n = k_w] = w[k][n]: k_conv_prep with one tap).
int linear_prep(const float* w, int K_w, int N_w, int mode, unsigned short* wop, hipStream_t s) {
    const int K = mode == 0 ? K_w : N_w, N = mode == 0 ? N_w : K_w;
    if (K % 16 != 0) {               // (mode 0 only: the callers hold mode 1's inner dimension to 16)
        hipLaunchKernelGGL(k_linear_prep_tail, dim3(64), dim3(256), 0, s, w, N_w, K_w, (K_w + 15) / 16 * 16, wop);
        AURPPO_LAUNCH_CHECK("k_linear_prep_tail");
        return AURPPO_OK;
    }
    hipLaunchKernelGGL(k_conv_prep, dim3(64), dim3(256), 0, s, w, N_w, K_w, K, N, mode, wop, 1);
    AURPPO_LAUNCH_CHECK("k_conv_prep");
    return AURPPO_OK;
}
// the same copy for a product of Kg x Ng that is wider than its weight (k_linear_prep_pad; Kg may be ragged as above: the product runs
// on the tail builds, and the copy has whole k-steps)
int linear_prep_pad(const float* w, int K_w, int N_w, int mode, int Kg, int Ng, unsigned short* wop, hipStream_t s) {
    hipLaunchKernelGGL(k_linear_prep_pad, dim3(64), dim3(256), 0, s, w, N_w, K_w, mode, (Kg + 15) / 16 * 16, Ng, wop);
    AURPPO_LAUNCH_CHECK("k_linear_prep_pad");
    return AURPPO_OK;
}
// the fold of (S, Np, Kp) slices into the (Nr, Kr) matrix `out` (k_fold_slices_pad; db != nullptr: the Nr bias gradients too)
int fold_slices_pad_launch(const float* part, int S, int Np, int Kp, int Nr, int Kr, float* out, const double* bpart, float* db, hipStream_t s) {
    const long long n_fold = ((long long)Nr * Kr + 255) / 256;
    hipLaunchKernelGGL(k_fold_slices_pad, dim3((unsigned)(n_fold + (db ? (Nr + 255) / 256 : 0))), dim3(256), 0, s, part, S, (long long)Np * Kp, Kp,
                       Nr, Kr, out, bpart, Np, db);
    AURPPO_LAUNCH_CHECK("k_fold_slices_pad");
    return AURPPO_OK;
}
int fold_slices_launch(const float* part, int S, long long n, float* out, const double* bpart, int N, float* db, hipStream_t s) {
    const long long n_fold = (n + 255) / 256;
    if (db) hipLaunchKernelGGL(k_fold_slices_bias, dim3((unsigned)(n_fold + (N + 255) / 256)), dim3(256), 0, s, part, S, n, out, bpart, N, db);
    else hipLaunchKernelGGL(k_fold_slices, dim3((unsigned)n_fold), dim3(256), 0, s, part, S, n, out);
    AURPPO_LAUNCH_CHECK("k_fold_slices");
    return AURPPO_OK;
}

// ---- weight gradients: the inner dimension (the minibatch's rows / the batch's output pixels) is cut into S slices, the slices'
// partial results land in the caller's workspace and k_fold_slices sums them in slice order.
// The slice count for `tiles` output tiles: the weight-gradient kernels hold two workgroups per CU (LDS), so the grid is dealt in
// rounds of 2 x 256 workgroups and a round with two workgroups in it costs what a full one does (1026 workgroups measured 611 us
// where 504 take 410): the S <= most that wastes the least of its last round, the smallest such S (fewer partial filters to fold).
int slices_for(long long tiles, long long most) {
    constexpr long long kSlots = 2 * 256;
    if (most < 1) most = 1;
    if (most > 4096) most = 4096;
    long long best = 1;
    double best_util = 0.0;
    for (long long S = 1; S <= most && tiles * S <= 4 * kSlots; ++S) {
        const long long wgs = tiles * S, rounds = (wgs + kSlots - 1) / kSlots;
        const double util = (double)wgs / (double)(rounds * kSlots);
        if (util > best_util + 0.02) {
            best_util = util;
            best = S;
        }
    }
    return (int)best;
}

extern "C" size_t aurppo_conv3x3_wop_bytes(int cin_gemm, int cout_gemm) {
    const size_t nblk = (size_t)((cout_gemm + 31) / 32 + kNBW);      // (+ one group of slack: a wave reads whole groups)
    return nblk * 9 * (size_t)((cin_gemm + 15) / 16) * 3 * 1024 + 64;      // (whole k-steps: a linear product's K may be ragged)
}

// mode 0: z = conv2d(x, w, padding = pad)                      x (B, Ci, H, W), w (Co, Ci, 3, 3), z (B, Co, H + 2 pad - 2, ...)
// mode 1: z = d conv2d / d input applied to x:  x (B, Co, Ho, Wo) is the output gradient, z (B, Ci, Ho + 2 - 2 pad, ...) the
//         input gradient, w the SAME (Co, Ci, 3, 3) filter, pad the FORWARD padding.
extern "C" int aurppo_conv3x3_f32(const float* x, const float* w, float* z, int B, int Ci_w, int Co_w, int H, int W, int pad,
                                  int mode, void* wop_ws, void* stream) {
    AURPPO_REQUIRE(mode == 0 || mode == 1, AURPPO_EINVAL, "aurppo_conv3x3_f32: mode %d", mode);
    const int cin = mode == 0 ? Ci_w : Co_w, cout = mode == 0 ? Co_w : Ci_w, p = mode == 0 ? pad : 2 - pad;
    return conv_fwd("aurppo_conv3x3_f32", false, false, x, nullptr, w, nullptr, z, nullptr, nullptr, wop_ws, B, cin, cout, H, W, p, Co_w,
                    Ci_w, mode, (hipStream_t)stream);
}

// K11p: y, mask = max_pool2d(relu(conv2d(x, w, padding = pad) + bias[c]), 2) with K9's semantics; x (B, Ci, H, W), w (Co, Ci, 3, 3),
// y / mask (B, Co, (H + 2 pad - 2) >> 1, (W + 2 pad - 2) >> 1).  Refuses what mode 0 above refuses, and a map without a whole window.
extern "C" int aurppo_conv3x3_pool_f32(const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int Ci,
                                       int Co, int H, int W, int pad, void* wop_ws, void* stream) {
    return conv_fwd("aurppo_conv3x3_pool_f32", true, false, x, nullptr, w, bias, y, mask, nullptr, wop_ws, B, Ci, Co, H, W, pad, Co, Ci, 0,
                    (hipStream_t)stream);
}

// ---- K11x: activations as bf16 planes (include/aurppo.h: the layout, and what each entry refuses)
extern "C" size_t aurppo_planes_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || C % 8 != 0) return 0;
    return (size_t)6 * B * C * H * W;
}

extern "C" int aurppo_split_planes_f32(const float* x, uint16_t* xp, int B, int C, int H, int W, void* stream) {
    AURPPO_REQUIRE(x && xp, AURPPO_EINVAL, "aurppo_split_planes_f32: null pointer");
    AURPPO_REQUIRE(aligned_to(xp, 16), AURPPO_EINVAL, "aurppo_split_planes_f32: planes not 16-byte aligned");
    AURPPO_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && C % 8 == 0 && (size_t)H * W < ((size_t)1 << 31) &&
                   (size_t)B * C * H * W < ((size_t)1 << 40), AURPPO_ESHAPE,
                   "aurppo_split_planes_f32: B=%d C=%d H=%d W=%d (C a multiple of 8)", B, C, H, W);
    const long long n_groups = (long long)B * (C / 8), total = n_groups * H * W;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_split_planes, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, x, xp, n_groups, H * W);
    AURPPO_LAUNCH_CHECK("k_split_planes");
    return AURPPO_OK;
}

// K11 on planes: z = conv2d(x, w, padding = pad) for the x whose planes xp holds -- aurppo_conv3x3_f32's mode 0, bit for bit.
extern "C" int aurppo_conv3x3_planes_f32(const uint16_t* xp, const float* w, float* z, int B, int Ci, int Co, int H, int W, int pad,
                                         void* wop_ws, void* stream) {
    return conv_fwd("aurppo_conv3x3_planes_f32", false, true, nullptr, xp, w, nullptr, z, nullptr, nullptr, wop_ws, B, Ci, Co, H, W, pad, Co,
                    Ci, 0, (hipStream_t)stream);
}

// K11p with its input read as planes (x_is_planes), its pooled output also written as planes (yp), or both; neither: K11p itself.
extern "C" int aurppo_conv3x3_pool_planes_f32(const void* x_or_xp, int x_is_planes, const float* w, const float* bias, float* y,
                                              uint8_t* mask, uint16_t* yp_or_null, int B, int Ci, int Co, int H, int W, int pad,
                                              void* wop_ws, void* stream) {
    if (!x_is_planes && !yp_or_null)
        return aurppo_conv3x3_pool_f32(reinterpret_cast<const float*>(x_or_xp), w, bias, y, mask, B, Ci, Co, H, W, pad, wop_ws, stream);
    const float* const x = x_is_planes ? nullptr : reinterpret_cast<const float*>(x_or_xp);
    const unsigned short* const xp = x_is_planes ? reinterpret_cast<const unsigned short*>(x_or_xp) : nullptr;
    return conv_fwd("aurppo_conv3x3_pool_planes_f32", true, true, x, xp, w, bias, y, mask, yp_or_null, wop_ws, B, Ci, Co, H, W, pad, Co, Ci, 0,
                    (hipStream_t)stream);
}

// K12: dw (Co, Ci, 3, 3) = the gradient of conv2d(x (B, Ci, H, W), w, padding = pad) with respect to w, given the output gradient
// dy (B, Co, H + 2 pad - 2, W + 2 pad - 2).  NCHW fp32.
namespace {
struct ConvWgradPlan {
    int WM, n_tiles_m, n_tiles_n, S, px_per_slice;
};
bool conv_wgrad_plan(int B, int Ci, int Co, int H, int W, int pad, ConvWgradPlan* p) {
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    if (B <= 0 || Ci <= 0 || Co <= 0 || Ho <= 0 || Wo <= 0 || pad < 0 || pad > 2) return false;
    const long long M = (long long)B * Ho * Wo, HoWo = (long long)Ho * Wo, HW = (long long)H * W;
    const int NK = Ci * 9;
    p->WM = Co > 64 ? 2 : 1;
    p->n_tiles_m = (Co + 64 * p->WM - 1) / (64 * p->WM);
    p->n_tiles_n = (NK + 64 * (4 / p->WM) - 1) / (64 * (4 / p->WM));
    const long long tiles = (long long)p->n_tiles_m * p->n_tiles_n;
    long long S = slices_for(tiles, (M + 511) / 512);       // at least 16 chunks of 32 pixels per slice
    long long pps = ((M + S - 1) / S + 31) / 32 * 32;
    // 32-bit offsets relative to the slice's first image: the images a slice touches must span less than 2^31 bytes of either tensor
    const long long per_img = 4 * (HoWo * Co > HW * Ci ? HoWo * Co : HW * Ci);
    if (per_img * 2 >= (1ll << 31)) return false;
    // ... and its pixel indices, counted from the first pixel of its first image, must stay exact in fp32 (the kernel's divisions)
    while (pps > 32 && ((pps / HoWo + 2) * per_img >= (1ll << 31) || pps + HoWo >= (1ll << 23))) pps = (pps / 2 + 31) / 32 * 32;
    if ((pps / HoWo + 2) * per_img >= (1ll << 31) || pps + HoWo >= (1ll << 23)) return false;
    S = (M + pps - 1) / pps;
    if (S * tiles >= (1ll << 31) || S > (1 << 20)) return false;
    p->S = (int)S;
    p->px_per_slice = (int)pps;
    return true;
}
}  // namespace

extern "C" size_t aurppo_conv3x3_wgrad_ws_bytes(int B, int Ci, int Co, int H, int W, int pad) {
    ConvWgradPlan p;
    if (!conv_wgrad_plan(B, Ci, Co, H, W, pad, &p)) return 0;
    return (size_t)p.S * (size_t)Co * (size_t)Ci * 9 * sizeof(float) + 64;
}

extern "C" int aurppo_conv3x3_wgrad_f32(const float* dy, const float* x, float* dw, int B, int Ci, int Co, int H, int W, int pad,
                                        void* ws, void* stream) {
    AURPPO_REQUIRE(dy && x && dw && ws, AURPPO_EINVAL, "aurppo_conv3x3_wgrad_f32: null pointer");
    ConvWgradPlan p;
    AURPPO_REQUIRE(conv_wgrad_plan(B, Ci, Co, H, W, pad, &p), AURPPO_ESHAPE,
                   "aurppo_conv3x3_wgrad_f32: B=%d Ci=%d Co=%d H=%d W=%d pad=%d (pad 0..2, non-empty output, one image of either tensor "
                   "under 1 GB)", B, Ci, Co, H, W, pad);
    AURPPO_REQUIRE(aligned_to(ws, 16), AURPPO_EINVAL, "aurppo_conv3x3_wgrad_f32: workspace not 16-byte aligned");
    ConvWgradArgs a;
    a.dy = dy; a.x = x; a.part = reinterpret_cast<float*>(ws);
    a.B = B; a.Ci = Ci; a.H = H; a.W = W; a.Co = Co; a.Ho = H + 2 * pad - 2; a.Wo = W + 2 * pad - 2; a.pad = pad;
    a.M = (long long)B * a.Ho * a.Wo;
    a.NK = Ci * 9;
    a.px_per_slice = p.px_per_slice;
    a.n_tiles_m = p.n_tiles_m; a.n_tiles_n = p.n_tiles_n;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g((unsigned)((long long)p.n_tiles_m * p.n_tiles_n * p.S)), blk(kConvThreads);
    // a quad of output pixels stays inside one row of its image, whose 16-byte pieces are aligned
    const bool quad = a.Wo % 4 == 0 && W >= 4 && pad <= 1 && aligned_to(dy, 16);
    if (p.WM == 2 && quad) hipLaunchKernelGGL((k_conv3x3_wgrad<2, true>), g, blk, 0, st, a);
    else if (p.WM == 2) hipLaunchKernelGGL((k_conv3x3_wgrad<2, false>), g, blk, 0, st, a);
    else if (quad) hipLaunchKernelGGL((k_conv3x3_wgrad<1, true>), g, blk, 0, st, a);
    else hipLaunchKernelGGL((k_conv3x3_wgrad<1, false>), g, blk, 0, st, a);
    AURPPO_LAUNCH_CHECK("k_conv3x3_wgrad");
    return fold_slices_launch(a.part, p.S, (long long)Co * a.NK, dw, nullptr, 0, nullptr, st);
}
