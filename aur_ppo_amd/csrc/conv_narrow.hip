// K11n / K12n -- the two gradients of the encoder's first hidden block, nn.Conv2d(16, 32, 3, padding=1) (src/nets/base_cnns.py:32-33),
// on the arithmetic of bf16x3.h in 16 x 16 x 32 matrix blocks.  K11 (conv.hip) works in 32-channel output blocks, of which an input
// gradient with 16 channels fills half; K12's smallest tile is 64 x 256, of which the 32 x 144 filter fills 28 %.  Both products here
// are shaped to the block: at most 16 input channels, 32 output channels per k-step (K11n) or in all (K12n).
//
// Arithmetic: three bf16 planes per fp32 operand, the six products of mma16x3 in its order, fp32 accumulation.  As in K11 / K12
// (bf3_gemm.h::mma32x3_step) a k-step's six products are summed from zero and the step's sum is added to the running accumulator once,
// and every other k-step runs negated, so that the matrix pipe's one-sided cut cancels between neighbours.  The negation costs nothing
// in the loop: it is applied to the fp32 value BEFORE it is split (the split of -a is the negated split of a).
//
// K11n  k_conv3x3_narrow_dgrad: dx (B, Ci <= 16, H, W) from dy (B, Co = 32 k, Ho, Wo) and w (Co, Ci, 3, 3).
//   GEMM per tap: C[m = ci][n = pixel] += A[m = ci][k = co] . B[k = co][n = pixel + tap]; a k-step is the 32 channels of one tap.
//   * a workgroup (4 waves) owns a tile of 8 rows x 16 columns of one image's dx; the dy tile with its one-pixel halo (10 x 18 pixels
//     x 32 channels) is split ONCE into three LDS planes, channel-minor, and serves all nine taps: a tap is a shift of the pixel row a
//     lane reads its 8 channels (one ds_read_b128 per plane) from.  K11 splits every value once per tap;
//   * the whole filter operand of 32 channels (9 taps x 3 planes x 1 KB = 27 KB, written in operand order by k_conv3x3_narrow_prep)
//     is copied into LDS once per workgroup (Co = 32) and stays there while the workgroup walks its tiles: no filter stream and no
//     barrier inside the tap loop.  With Co > 32 both are staged again per group of 32 channels;
//   * the next tile's values are requested before a tile's tap loop and split after it: two workgroups a CU hide no load latency;
//   * the accumulator has the pixel on the lane: a store is 16 consecutive pixels of one channel per quarter wave.
//   Addresses into dy and dx are 64-bit; zero padding, the halo outside the map and pixels outside the image are zeros in LDS / skipped
//   stores, never an access.
//
// K12n  k_conv3x3_narrow_wgrad: dw (Co <= 32, Ci <= 16, 3, 3) from dy and x.
//   C[m = co][n = ci * 9 + tap] = sum over output pixels: 2 x 9 blocks of 16 x 16 = 72 accumulator registers, so ONE WAVE owns the
//   whole filter and a slice of the batch's pixels of its own: a workgroup is a wave, there is no workgroup barrier to wait at, and the
//   S slices' partial filters are folded in slice order by k_fold_slices (conv.hip), as K12's are.  Per chunk of 32 pixels the wave
//   stages its 32 dy rows and 144 (ci, tap) rows of x into one F image (bf16x3.h) and reads every fragment along a row.  Loads are K12's:
//   buffer loads with 32-bit offsets relative to the slice's first image, a per-chunk table of pixel offsets per tap in LDS, an offset
//   past the buffer for whatever is outside (the hardware returns 0).  (K12's QUAD form -- one 16-byte load per row and pixel quad -- was built and measured slower here)  The next chunk's values are in flight while this one multiplies.
#pragma clang fp contract(fast)
#include "bf3_gemm.h"
#include "common.h"

using namespace bf3;

namespace {

// ------------------------------------------------------------------------------------------------------------------- K11n
constexpr int kNdTileH = 8, kNdTileW = 16;                       // dx pixels of a tile
constexpr int kNdHaloW = kNdTileW + 2, kNdHaloPx = (kNdTileH + 2) * kNdHaloW;      // 18, 180
constexpr int kNdPxRow = 80;                                     // bytes per halo pixel and plane: 32 channels + 16 (stride 20 banks)
constexpr int kNdDyPlane = kNdHaloPx * kNdPxRow;                 // 14 400
constexpr int kNdWBytes = 9 * 3 * 1024;                          // the filter operand of 32 channels: [tap][plane][lane][8] bf16
constexpr int kNdLds = kNdWBytes + 3 * kNdDyPlane;               // 70 848: two workgroups per CU
constexpr int kNdMaxGrid = 2048;

struct NarrowDgradArgs {
    const float* dy;                 // (B, Co, Ho, Wo)
    const unsigned short* wop;       // [Co / 32][tap][plane][lane][8]
    float* dx;                       // (B, Ci, H, W)
    int B, Ci, Co, H, W, Ho, Wo;
    int q;                           // the product's own padding, 2 - pad
    int CG;                          // Co / 32
    int tiles_y, tiles_x;
    long long n_tiles;               // B * tiles_y * tiles_x
};

// w (Co, Ci, 3, 3) -> A[m = ci][k = co] per product tap (the filter's tap flipped), lane l holding m = l & 15, k = 8 (l >> 4) + j;
// rows ci >= Ci are zero; odd taps are stored negated (the kernel subtracts their step).
__global__ __launch_bounds__(256) void k_conv3x3_narrow_prep(const float* __restrict__ w, int Ci, int CG, unsigned short* __restrict__ wop) {
    const int total = CG * 9 * 512;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int j = e & 7, lane = (e >> 3) & 63, r = e >> 9;
        const int cg = r / 9, tap = r - 9 * cg;
        const int ci = lane & 15, co = cg * 32 + 8 * (lane >> 4) + j;
        float v = ci < Ci ? w[((size_t)co * Ci + ci) * 9 + (8 - tap)] : 0.0f;
        if (tap & 1) v = -v;
        unsigned p0, p1, p2;
        split3(v, 0.0f, p0, p1, p2);
        const size_t at = ((size_t)r * 3 * 64 + lane) * 8 + j;
        wop[at] = (unsigned short)p0;
        wop[at + 512] = (unsigned short)p1;
        wop[at + 1024] = (unsigned short)p2;
    }
}

__global__ __launch_bounds__(kConvThreads, 2) void k_conv3x3_narrow_dgrad(const NarrowDgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char s_nd[];
    char* const s_w = s_nd;
    char* const s_dy = s_nd + kNdWBytes;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    const int HoWo = a.Ho * a.Wo;
    const int per_img = a.tiles_y * a.tiles_x;
    // a stage = one tile's 32 channels of group cg.  A thread takes kNdIters halo pixels of a channel pair each (consecutive lanes:
    // consecutive pixels); ALL of a stage's loads are issued before the tap loop of the stage in front of it, and split after it
    constexpr int kNdIters = (16 * kNdHaloPx + kConvThreads - 1) / kConvThreads;       // 12 (the last one for 64 threads)
    float v0[kNdIters], v1[kNdIters];
    auto request = [&](long long tile, int cg) {
        const int b = (int)(tile / per_img), rem = (int)(tile - (long long)b * per_img);
        const int tyi = rem / a.tiles_x, txi = rem - tyi * a.tiles_x;
        const int y0 = tyi * kNdTileH, x0 = txi * kNdTileW;
        const float* const dyb = a.dy + (size_t)b * a.Co * HoWo + (size_t)(cg * 32) * HoWo;
#pragma unroll
        for (int k = 0; k < kNdIters; ++k) {
            const int i = tid + k * kConvThreads;
            const int cp = i / kNdHaloPx, t = i - cp * kNdHaloPx;
            const int r = t / kNdHaloW, c = t - r * kNdHaloW;
            const int yy = y0 - a.q + r, xx = x0 - a.q + c;
            v0[k] = 0.0f;
            v1[k] = 0.0f;
            if (i < 16 * kNdHaloPx && yy >= 0 && yy < a.Ho && xx >= 0 && xx < a.Wo) {
                const float* const p = dyb + (size_t)(2 * cp) * HoWo + (yy * a.Wo + xx);
                v0[k] = p[0];
                v1[k] = p[HoWo];
            }
        }
    };
    auto place = [&]() {
#pragma unroll
        for (int k = 0; k < kNdIters; ++k) {
            const int i = tid + k * kConvThreads;
            const int cp = i / kNdHaloPx, t = i - cp * kNdHaloPx;
            unsigned p0, p1, p2;
            split3(v0[k], v1[k], p0, p1, p2);
            const int o = t * kNdPxRow + cp * 4;
            if (i < 16 * kNdHaloPx) {
                *reinterpret_cast<unsigned*>(s_dy + 0 * kNdDyPlane + o) = p0;
                *reinterpret_cast<unsigned*>(s_dy + 1 * kNdDyPlane + o) = p1;
                *reinterpret_cast<unsigned*>(s_dy + 2 * kNdDyPlane + o) = p2;
            }
        }
    };
    bool have_w = false;
    long long tile = blockIdx.x;
    int cg = 0;
    f32x4v acc[2];
    if (tile < a.n_tiles) request(tile, 0);
    while (tile < a.n_tiles) {
        __syncthreads();                                    // the previous stage has been read
        if (!have_w || a.CG > 1) {
            const u32x4* const src = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.wop) + (size_t)cg * kNdWBytes);
            for (int i = tid; i < kNdWBytes / 16; i += kConvThreads) reinterpret_cast<u32x4*>(s_w)[i] = src[i];
            have_w = true;
        }
        place();
        __syncthreads();
        long long next_tile = tile;
        int next_cg = cg + 1;
        if (next_cg == a.CG) {
            next_cg = 0;
            next_tile += gridDim.x;
        }
        if (next_tile < a.n_tiles) request(next_tile, next_cg);      // in flight while this stage multiplies
        if (cg == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ty = tap / 3, tx = tap - 3 * ty;
            Frag3 A;
#pragma unroll
            for (int p = 0; p < 3; ++p) A.p[p] = lds_b128(s_w + (tap * 3 + p) * 1024 + lane * 16);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int t = (2 * w + blk + ty) * kNdHaloW + n + tx;
                Frag3 Bf;
#pragma unroll
                for (int p = 0; p < 3; ++p) Bf.p[p] = lds_b128(s_dy + p * kNdDyPlane + t * kNdPxRow + g * 16);
                const f32x4v st = mma16x3(A, Bf, f32x4v{0.0f, 0.0f, 0.0f, 0.0f});
                acc[blk] = (tap & 1) ? acc[blk] - st : acc[blk] + st;
            }
        }
        if (cg == a.CG - 1) {
            // C[m = ci = 4 g + e][n = pixel]: 16 consecutive pixels of a channel per quarter wave
            const int b = (int)(tile / per_img), rem = (int)(tile - (long long)b * per_img);
            const int tyi = rem / a.tiles_x, txi = rem - tyi * a.tiles_x;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int y = tyi * kNdTileH + 2 * w + blk, x = txi * kNdTileW + n;
                if (y < a.H && x < a.W) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ci = 4 * g + e;
                        if (ci < a.Ci) a.dx[((size_t)(b * (long long)a.Ci + ci) * a.H + y) * a.W + x] = acc[blk][e];
                    }
                }
            }
        }
        tile = next_tile;
        cg = next_cg;
    }
}

// ------------------------------------------------------------------------------------------------------------------- K12n
constexpr int kNwRows = 32 + 144, kNwSlots = kNwRows / 8;       // image rows: 32 dy channels, 144 filter columns; rows per lane
constexpr int kNwPlane = kNwRows * kFRow;                        // 11 264 bytes
constexpr unsigned kNwOob = 0x80000000u;                         // buffer offsets from here on read 0 (num_records <= 2^31)
constexpr long long kNwSlices = 2048;                            // slices aimed at: two rounds of four one-wave workgroups per CU (LDS)

struct NarrowWgradArgs {
    const float* dy;                 // (B, Co, Ho, Wo)
    const float* x;                  // (B, Ci, H, W)
    float* part;                     // (S, Co, Ci * 9)
    int B, Ci, H, W, Co, Ho, Wo, pad;
    long long M;                     // B * Ho * Wo
    int NK;                          // Ci * 9
    int px_per_slice;                // a multiple of 32
};

__global__ __launch_bounds__(64) void k_conv3x3_narrow_wgrad(const NarrowWgradArgs a) {
    __shared__ __attribute__((aligned(16))) char s_img[3 * kNwPlane];
    // per chunk (two in flight): row 0 = the dy offsets of its 32 pixels, rows 1..9 = the x offsets per tap; kNwOob where a pixel is
    // past the slice or a tap outside the image
    __shared__ __attribute__((aligned(16))) unsigned s_tab[2][10][32];
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    const int HoWo = a.Ho * a.Wo, HW = a.H * a.W;
    const long long m_lo = (long long)s * a.px_per_slice;
    long long m_hi = m_lo + a.px_per_slice;
    if (m_hi > a.M) m_hi = a.M;
    const int n_px = (int)(m_hi - m_lo);
    const int b_lo = (int)(m_lo / HoWo), r_lo = (int)(m_lo - (long long)b_lo * HoWo);
    // buffers that start at the slice's first image
    const size_t left_a = (size_t)(a.B - b_lo) * a.Co * HoWo * 4, left_b = (size_t)(a.B - b_lo) * a.Ci * HW * 4;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy + (size_t)b_lo * a.Co * HoWo), 0, (unsigned)(left_a < kNwOob ? left_a : kNwOob), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x + (size_t)b_lo * a.Ci * HW), 0, (unsigned)(left_b < kNwOob ? left_b : kNwOob), 0x00020000);
    // this lane's image rows (crow + 8 u) and its pixel quad.  Rows past the tensor (channels >= Co, columns >= Ci * 9) are staged from
    // beyond the buffer or from wherever a wrapped offset lands: their products are never stored
    const int q4 = (lane & 7) * 4, crow = lane >> 3;
    unsigned row_off[kNwSlots];
    int row_tap[kNwSlots];
#pragma unroll
    for (int u = 0; u < kNwSlots; ++u) {
        const int row = crow + 8 * u;
        if (u < 4) {
            row_off[u] = row < a.Co ? (unsigned)row * (unsigned)HoWo * 4u : kNwOob;
            row_tap[u] = 0;
        } else {
            const int nn = row - 32, ci = nn / 9;
            row_off[u] = nn < a.NK ? (unsigned)(ci * HW) * 4u : kNwOob;
            row_tap[u] = 1 + (nn - 9 * ci);
        }
    }
    const float inv_howo = 1.0f / (float)HoWo, inv_wo = 1.0f / (float)a.Wo;
    auto fdiv = [](int nn, int d, float inv, int& rem) {       // (the slice's pixel indices stay below 2^23: narrow_wgrad_plan)
        int q = (int)((float)nn * inv);
        int r = nn - q * d;
        if (r < 0) { q -= 1; r += d; }
        else if (r >= d) { q += 1; r -= d; }
        rem = r;
        return q;
    };
    auto table = [&](int c) {
        if (lane < 32) {
            const int i = c * 32 + lane;
            unsigned (*const tab)[32] = s_tab[c & 1];
            int r, x;
            const int b = fdiv(r_lo + i, HoWo, inv_howo, r);        // (relative to the first pixel of image b_lo)
            const int y = fdiv(r, a.Wo, inv_wo, x);
            const int base = b * a.Ci * HW + (y - a.pad) * a.W + (x - a.pad);
            const bool live = i < n_px;
            tab[0][lane] = live ? (unsigned)(b * a.Co * HoWo + r) * 4u : kNwOob;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t - 3 * ky;
                const int iy = y + ky - a.pad, ix = x + kx - a.pad;
                const bool in = live && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                tab[1 + t][lane] = in ? (unsigned)(base + ky * a.W + kx) * 4u : kNwOob;
            }
        }
    };
    float v[kNwSlots][4];
    auto fetch = [&](int c) {
        const unsigned (*const tab)[32] = s_tab[c & 1];
#pragma unroll
        for (int u = 0; u < kNwSlots; ++u) {
            const u32x4 t = *reinterpret_cast<const u32x4*>(&tab[row_tap[u]][q4]);        // this row's offsets of the quad's pixels
            const __amdgpu_buffer_rsrc_t r = u < 4 ? ra : rb;
            v[u][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.x + row_off[u], 0, 0));
            v[u][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.y + row_off[u], 0, 0));
            v[u][2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.z + row_off[u], 0, 0));
            v[u][3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.w + row_off[u], 0, 0));
        }
    };
    f32x4v acc[2][9];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[i][j] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    const int n_chunks = (n_px + 31) >> 5;
    // one chunk: its values (requested a chunk ago) -> planes -> products; meanwhile the next chunk is requested into the same registers.
    // (__syncthreads in a one-wave workgroup orders the wave's own LDS traffic; nobody waits for anybody.)
    auto step = [&](int c, auto neg) {
        constexpr bool NEG = decltype(neg)::value;
        __syncthreads();                                    // the previous chunk's fragments have been read
#pragma unroll
        for (int u = 0; u < kNwSlots; ++u) {
            float x0 = v[u][0], x1 = v[u][1], x2 = v[u][2], x3 = v[u][3];
            if (NEG && u < 4) { x0 = -x0; x1 = -x1; x2 = -x2; x3 = -x3; }      // (the dy rows: the A operand comes negated)
            unsigned a0, a1, a2, b0, b1, b2;
            split3(x0, x1, a0, a1, a2);
            split3(x2, x3, b0, b1, b2);
            const int o = foff(crow + 8 * u, q4);
            *reinterpret_cast<u32x2*>(s_img + 0 * kNwPlane + o) = u32x2{a0, b0};
            *reinterpret_cast<u32x2*>(s_img + 1 * kNwPlane + o) = u32x2{a1, b1};
            *reinterpret_cast<u32x2*>(s_img + 2 * kNwPlane + o) = u32x2{a2, b2};
        }
        __syncthreads();
        if (c + 1 < n_chunks) fetch(c + 1);
        if (c + 2 < n_chunks) table(c + 2);                 // (slot c & 1: last read by fetch(c), before this chunk's barriers)
        const Frag3 A0 = f_rows16<kNwPlane>(s_img, 0, lane), A1 = f_rows16<kNwPlane>(s_img, 16, lane);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const Frag3 Bf = f_rows16<kNwPlane>(s_img, 32 + 16 * j, lane);
            const f32x4v t0 = mma16x3(A0, Bf, f32x4v{0.0f, 0.0f, 0.0f, 0.0f});
            const f32x4v t1 = mma16x3(A1, Bf, f32x4v{0.0f, 0.0f, 0.0f, 0.0f});
            acc[0][j] = NEG ? acc[0][j] - t0 : acc[0][j] + t0;
            acc[1][j] = NEG ? acc[1][j] - t1 : acc[1][j] + t1;
        }
    };
    table(0);
    if (n_chunks > 1) table(1);
    __syncthreads();
    fetch(0);
    for (int c = 0; c < n_chunks; c += 2) {
        step(c, std::false_type{});
        if (c + 1 < n_chunks) step(c + 1, std::true_type{});
    }
    // C[m = co = 16 i + 4 (lane >> 4) + e][n = 16 j + (lane & 15)]: rows of `part` are contiguous over the lanes
    float* const out = a.part + (size_t)s * a.Co * a.NK;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int col = 16 * j + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 16 * i + 4 * (lane >> 4) + e;
                if (row < a.Co && col < a.NK) out[(size_t)row * a.NK + col] = acc[i][j][e];
            }
        }
}

bool narrow_class(int Ci, int Co_max, int Co, bool co_blocks, int pad) {
    if (Ci < 1 || Ci > 16 || Co < 1 || pad < 0 || pad > 2) return false;
    return co_blocks ? Co % 32 == 0 : Co <= Co_max;
}

// K12n's slices: about kNwSlices of them, at least 16 chunks of 32 pixels each, cut further until a slice's images span less than
// 2^31 bytes of either tensor and its pixel indices stay exact in fp32 (the kernel's divisions) -- conv_wgrad_plan's rules.
struct NarrowWgradPlan {
    int S, px_per_slice;
};
bool narrow_wgrad_plan(int B, int Ci, int Co, int H, int W, int pad, NarrowWgradPlan* p) {
    if (!narrow_class(Ci, 32, Co, false, pad) || B <= 0 || H <= 0 || W <= 0) return false;
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    if (Ho <= 0 || Wo <= 0) return false;
    const long long M = (long long)B * Ho * Wo, HoWo = (long long)Ho * Wo, HW = (long long)H * W;
    long long pps = (M + kNwSlices - 1) / kNwSlices;
    if (pps < 512) pps = 512;
    pps = (pps + 31) / 32 * 32;
    const long long per_img = 4 * (HoWo * Co > HW * Ci ? HoWo * Co : HW * Ci);
    if (per_img * 2 >= (1ll << 31)) return false;
    while (pps > 32 && ((pps / HoWo + 2) * per_img >= (1ll << 31) || pps + HoWo >= (1ll << 23))) pps = (pps / 2 + 31) / 32 * 32;
    if ((pps / HoWo + 2) * per_img >= (1ll << 31) || pps + HoWo >= (1ll << 23)) return false;
    const long long S = (M + pps - 1) / pps;
    if (S > (1 << 20)) return false;
    p->S = (int)S;
    p->px_per_slice = (int)pps;
    return true;
}

}  // namespace

// K11n: dx (B, Ci, H, W) = d conv2d(x, w, padding = pad) / d x applied to dy (B, Co, H + 2 pad - 2, W + 2 pad - 2)
extern "C" size_t aurppo_conv3x3_dgrad_narrow_wop_bytes(int Ci, int Co) {
    if (!narrow_class(Ci, 0, Co, true, 0)) return 0;
    return (size_t)(Co / 32) * kNdWBytes;
}

extern "C" int aurppo_conv3x3_dgrad_narrow_f32(const float* dy, const float* w, float* dx, int B, int Ci, int Co, int H, int W, int pad,
                                               void* wop_ws, void* stream) {
    const char* const who = "aurppo_conv3x3_dgrad_narrow_f32";
    AURPPO_REQUIRE(dy && w && dx && wop_ws, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(narrow_class(Ci, 0, Co, true, pad), AURPPO_ESHAPE, "%s: Ci=%d (1..16) Co=%d (a multiple of 32) pad=%d (0..2)", who, Ci, Co, pad);
    AURPPO_REQUIRE(B > 0 && H > 0 && W > 0, AURPPO_ESHAPE, "%s: B=%d H=%d W=%d", who, B, H, W);
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    AURPPO_REQUIRE(Ho > 0 && Wo > 0, AURPPO_ESHAPE, "%s: empty output gradient (%d x %d)", who, Ho, Wo);
    AURPPO_REQUIRE((long long)Co * Ho * Wo < (1ll << 31) && (long long)H * W < (1ll << 27) &&
                       (size_t)B * Co * Ho * Wo < ((size_t)1 << 40) && (size_t)B * Ci * H * W < ((size_t)1 << 40),
                   AURPPO_ESHAPE, "%s: operand too large", who);
    AURPPO_REQUIRE(aligned_to(wop_ws, 16), AURPPO_EINVAL, "%s: workspace not 16-byte aligned", who);
    NarrowDgradArgs a;
    a.dy = dy; a.wop = reinterpret_cast<unsigned short*>(wop_ws); a.dx = dx;
    a.B = B; a.Ci = Ci; a.Co = Co; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.q = 2 - pad;
    a.CG = Co / 32;
    a.tiles_y = (H + kNdTileH - 1) / kNdTileH;
    a.tiles_x = (W + kNdTileW - 1) / kNdTileW;
    a.n_tiles = (long long)B * a.tiles_y * a.tiles_x;
    AURPPO_REQUIRE(a.n_tiles < (1ll << 31), AURPPO_ESHAPE, "%s: too many tiles", who);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_conv3x3_narrow_prep, dim3(a.CG < 8 ? 9 * a.CG : 72), dim3(256), 0, s, w, Ci, a.CG, reinterpret_cast<unsigned short*>(wop_ws));
    AURPPO_LAUNCH_CHECK("k_conv3x3_narrow_prep");
    const int grid = (int)(a.n_tiles < kNdMaxGrid ? a.n_tiles : kNdMaxGrid);
    return launch_dyn_lds<k_conv3x3_narrow_dgrad>("k_conv3x3_narrow_dgrad", grid, kConvThreads, kNdLds, kNdLds, s, a);
}

// K12n: dw (Co, Ci, 3, 3) = the gradient of conv2d(x (B, Ci, H, W), w, padding = pad) with respect to w under dy
extern "C" size_t aurppo_conv3x3_wgrad_narrow_ws_bytes(int B, int Ci, int Co, int H, int W, int pad) {
    NarrowWgradPlan p;
    if (!narrow_wgrad_plan(B, Ci, Co, H, W, pad, &p)) return 0;
    return (size_t)p.S * (size_t)Co * (size_t)Ci * 9 * sizeof(float);
}

extern "C" int aurppo_conv3x3_wgrad_narrow_f32(const float* dy, const float* x, float* dw, int B, int Ci, int Co, int H, int W, int pad,
                                               void* ws, void* stream) {
    const char* const who = "aurppo_conv3x3_wgrad_narrow_f32";
    AURPPO_REQUIRE(dy && x && dw && ws, AURPPO_EINVAL, "%s: null pointer", who);
    NarrowWgradPlan p;
    AURPPO_REQUIRE(narrow_wgrad_plan(B, Ci, Co, H, W, pad, &p), AURPPO_ESHAPE,
                   "%s: B=%d Ci=%d (1..16) Co=%d (1..32) H=%d W=%d pad=%d (0..2, non-empty output, one image of either tensor under 1 GB)",
                   who, B, Ci, Co, H, W, pad);
    AURPPO_REQUIRE(aligned_to(ws, 16), AURPPO_EINVAL, "%s: workspace not 16-byte aligned", who);
    NarrowWgradArgs a;
    a.dy = dy; a.x = x; a.part = reinterpret_cast<float*>(ws);
    a.B = B; a.Ci = Ci; a.H = H; a.W = W; a.Co = Co; a.Ho = H + 2 * pad - 2; a.Wo = W + 2 * pad - 2; a.pad = pad;
    a.M = (long long)B * a.Ho * a.Wo;
    a.NK = Ci * 9;
    a.px_per_slice = p.px_per_slice;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_conv3x3_narrow_wgrad, dim3((unsigned)p.S), dim3(64), 0, st, a);
    AURPPO_LAUNCH_CHECK("k_conv3x3_narrow_wgrad");
    return fold_slices_launch(a.part, p.S, (long long)Co * a.NK, dw, nullptr, 0, nullptr, st);
}
