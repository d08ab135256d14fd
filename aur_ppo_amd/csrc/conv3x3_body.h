// The body of k_conv3x3 (conv.hip), included INSIDE each of its two kernel templates: NB, BUF and POOL are compile-time constants of
// the including kernel, `a` its ConvArgs, `pool_bias` / `pool_mask` the POOL builds' two further arguments (null constants in the
// plain builds).  One text, so the two cannot drift; compiled in place, so the plain builds keep their names and their instruction
// streams (through a shared __device__ function they kept neither).
//
// POOL (K11p, behind aurppo_conv3x3_pool_f32): bias, ReLU and the 2 x 2 max-pool of K9 (csrc/pool.hip) in the epilogue.  The 32
// "pixels" of a block are 8 consecutive pooled windows q = (b, ho, wo), flattened over B * Ho * Wo (a.Ho x a.Wo is the POOLED map):
// lanes 0-15 the windows' upper rows (window l >> 1, column l & 1), lanes 16-31 the lower rows.  A window's four pre-activations
// then sit in ONE wave's LDS tile, and the pool needs no other wave, no further LDS and no atomics.  Every lane still derives its own
// (b, y, x): taps, offsets, the out-of-image handling and the matrix loop are the plain builds', for any map width, for windows
// that wrap rows or images inside a block, with buffer loads or 64-bit addresses.  Every accumulator element is formed by the
// same k-steps in the same order (kStepNeg depends on the k-step, not on the pixel), so it holds the very bits the plain build
// stores in z.  An odd trailing row / column belongs to no window and is never computed.
//
// XPL / OPL (K11x, behind aurppo_conv3x3_planes_f32 and aurppo_conv3x3_pool_planes_f32; constants of the including kernel like POOL, with
// `in_planes` / `out_planes` their two further arguments): activations kept as bf16 planes, include/aurppo.h's layout
// uint16 [b][channel group of 8][plane][pixel][8].  XPL: the A operand is READ as planes -- the 16 bytes at (b, group, plane, pixel) are
// the bf16x8 that lane (pixel, h) would have split from its 8 fp32 channels, so load_a is three 16-byte loads per pixel block and the
// split loop is gone; a tap outside the image reads zeros, which are split3(0.0f)'s planes.  The values that meet the matrix pipe are the
// same bits in the same order, so z (or y and the mask) holds what the fp32 build leaves.  OPL (with POOL): the epilogue also writes the
// pooled output's planes, split3 of the very value it stores in y.
    constexpr int kChunkBytes = kKC * NB * 3 * 1024;
    constexpr int kLdsBytes = 2 * kChunkBytes > (kConvThreads / kWave) * 32 * kTileLd * 4 ? 2 * kChunkBytes
                                                                                        : (kConvThreads / kWave) * 32 * kTileLd * 4;
    __shared__ __attribute__((aligned(16))) char s_b[kLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mb8 = (int)(blockIdx.x % (unsigned)a.n_mb4), ng = (int)(blockIdx.x / (unsigned)a.n_mb4);
    const int h = lane >> 5;
    const int HWo = a.Ho * a.Wo, HW = a.H * a.W;
    const int CG = a.CG, KS = 9 * CG;
    bool valid[kMB];
    int yy[kMB], xx[kMB];
    size_t img[kMB], out_px[kMB];
    [[maybe_unused]] size_t out_pl[kMB];      // OPL: the window's first element in the output planes
#pragma unroll
    for (int mb = 0; mb < kMB; ++mb) {
        if constexpr (POOL) {
            const int l = lane & 31;
            const long long q = (((long long)mb8 * 4 + w) * kMB + mb) * 8 + ((l & 15) >> 1);      // this lane's window
            valid[mb] = q < (a.M >> 2);
            int b = 0, r = 0, y = 0, x = 0;
            if (valid[mb]) {
                b = (int)(q / HWo);
                r = (int)(q - (long long)b * HWo);
                const int ho = r / a.Wo;
                y = 2 * ho + (l >> 4);
                x = 2 * (r - ho * a.Wo) + (l & 1);
            }
            yy[mb] = y; xx[mb] = x;
            if constexpr (XPL) img[mb] = (size_t)b * (a.Cin >> 3) * 3 * HW;      // in 16-byte pieces of the planes
            else img[mb] = (size_t)b * a.Cin * HW;
            out_px[mb] = (size_t)b * a.Cout * HWo + (size_t)r;       // the window's place in channel 0 of its image
            if constexpr (OPL) out_pl[mb] = ((size_t)b * (a.Cout >> 3) * 3 * HWo + (size_t)r) * 8;      // ... and in plane 0 of its image's group 0
        } else {
            const long long m = (((long long)mb8 * 4 + w) * kMB + mb) * 32 + (lane & 31);
            valid[mb] = m < a.M;
            int b = 0, y = 0, x = 0;
            if (valid[mb]) {
                b = (int)(m / HWo);
                const int r = (int)(m - (long long)b * HWo);
                y = r / a.Wo;
                x = r - y * a.Wo;
            }
            yy[mb] = y; xx[mb] = x;
            if constexpr (XPL) img[mb] = (size_t)b * (a.Cin >> 3) * 3 * HW;
            else img[mb] = (size_t)b * a.Cin * HW;
            out_px[mb] = (size_t)b * a.Cout * HWo + (size_t)(y * a.Wo + x);
        }
    }
    // the filter of this channel group: [nb][k-step][plane][lane][16 B]; a chunk = k-steps kc*kKC .. of every nb
    const char* const wgrp = reinterpret_cast<const char*>(a.wop) + (size_t)(ng * NB) * KS * 3 * 1024;
    // fragment f of a chunk (f = (kk * NB + nb) * 3 + plane): wave w brings fragments w, w + 4, ...
    auto stage = [&](int kc, int buf) {
        char* const dst = s_b + buf * kChunkBytes;
#pragma unroll
        for (int f = 0; f < kKC * NB * 3; ++f) {
            if ((f & 3) != w) continue;              // (wave-uniform)
            const int pl = f % 3, nb = (f / 3) % NB, kk = f / (3 * NB);
            const int ks = kc * kKC + kk;
            if (ks < KS) dma16(wgrp + ((size_t)(nb * KS + ks) * 3 + pl) * 1024 + lane * 16, dst + f * 1024);
        }
    };

    f32x16c acc[kMB][NB];
#pragma unroll
    for (int mb = 0; mb < kMB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mb][nb][e] = 0.0f;

    // the A values of one k-step: this lane's 8 channels of the tap's input pixel, for both pixel blocks -- fp32 values, or (XPL) their
    // three planes as they lie in memory, 16 bytes each (put_plane / get_plane, conv.hip: the buffer's type differs between the builds)
    using ABuf = std::conditional_t<XPL, u32x4[kMB][3], float[kMB][8]>;
    constexpr int kALoads = XPL ? 3 : 8;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        XPL ? (void*)const_cast<unsigned short*>(in_planes) : (void*)const_cast<float*>(a.x), 0,
        BUF ? (unsigned)((size_t)a.B * a.Cin * HW * (XPL ? 6 : 4)) : 0u, 0x00020000);
    unsigned pix_off[kMB];           // BUF: byte offset of (b, channel 8 h, y - pad, x - pad) -- may wrap below zero, used with a valid tap only
#pragma unroll
    for (int mb = 0; mb < kMB; ++mb) {
        if constexpr (XPL) pix_off[mb] = (unsigned)((img[mb] + (size_t)(3 * h) * HW) * 16) + (unsigned)(((yy[mb] - a.pad) * a.W + (xx[mb] - a.pad)) * 16);
        else pix_off[mb] = (unsigned)((img[mb] + (size_t)(8 * h) * HW) * 4) + (unsigned)(((yy[mb] - a.pad) * a.W + (xx[mb] - a.pad)) * 4);
    }
    auto load_a = [&](int ks, ABuf& v) {
        const int tap = ks / CG, cg = ks - tap * CG;
        const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            const int iy = yy[mb] + ky - a.pad, ix = xx[mb] + kx - a.pad;
            const bool inb = valid[mb] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            if constexpr (XPL) {
                // group 2 cg + h of the pixel's image: plane pl lies (6 cg + pl) * HW pieces behind plane 0 of group h
                if (BUF) {
                    const unsigned vo = inb ? pix_off[mb] + (unsigned)((ky * a.W + kx) * 16) : 0xfffffff0u;    // past the buffer: reads 0
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        put_plane(v[mb], pl, __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo, (6 * cg + pl) * HW * 16, 0)));
                } else {
                    const u32x4* const src = reinterpret_cast<const u32x4*>(in_planes);
                    const size_t at = img[mb] + (size_t)(6 * cg + 3 * h) * HW + (size_t)(inb ? iy * a.W + ix : 0);
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) {
                        const u32x4 t = src[inb ? at + (size_t)pl * HW : 0];
                        put_plane(v[mb], pl, inb ? t : u32x4{0u, 0u, 0u, 0u});
                    }
                }
            } else if (BUF) {
                const unsigned vo = inb ? pix_off[mb] + (unsigned)((ky * a.W + kx) * 4) : 0xfffffff0u;     // past the buffer: reads 0
                const int so0 = cg * 16 * HW * 4;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[mb][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, so0 + j * HW * 4, 0));
            } else {
                const size_t at = img[mb] + (size_t)(cg * 16 + 8 * h) * HW + (size_t)(inb ? iy * a.W + ix : 0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = a.x[inb ? at + (size_t)j * HW : 0];
                    v[mb][j] = inb ? t : 0.0f;
                }
            }
        }
    };
    const int n_chunks = (KS + kKC - 1) / kKC;
    ABuf abuf[2];                    // k-step ks computes from abuf[ks & 1] while abuf[(ks + 1) & 1] is in flight (kKC = 2: the parity is kk's)
    static_assert(kKC == 2, "the A registers ping-pong on the k-step's position inside its chunk");
    stage(0, 0);
    load_a(0, abuf[0]);
    static_assert(kMB * kALoads == (XPL ? 6 : 16), "the wait below counts load_a's loads");
    if constexpr (XPL) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");      // (the DMA pieces are older than the 16 loads of load_a)
    __syncthreads();
    for (int kc = 0; kc < n_chunks; ++kc) {
        if (kc + 1 < n_chunks) stage(kc + 1, (kc + 1) & 1);
        const char* const bsrc = s_b + (kc & 1) * kChunkBytes + lane * 16;
#pragma unroll
        for (int kk = 0; kk < kKC; ++kk) {
            const int ks = kc * kKC + kk;
            if (ks < KS) {
                ABuf& cur = abuf[kk];
                if (ks + 1 < KS) load_a(ks + 1, abuf[kk ^ 1]);
                Frag3 A[kMB];
#pragma unroll
                for (int mb = 0; mb < kMB; ++mb) {
                    if constexpr (XPL) {
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) A[mb].p[pl] = __builtin_bit_cast(bf16x8, get_plane(cur[mb], pl));
                    } else {
                        unsigned p[4][3];
#pragma unroll
                        for (int q = 0; q < 4; ++q) split3(cur[mb][2 * q], cur[mb][2 * q + 1], p[q][0], p[q][1], p[q][2]);
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) {
                            const u32x4 v = {p[0][pl], p[1][pl], p[2][pl], p[3][pl]};
                            A[mb].p[pl] = __builtin_bit_cast(bf16x8, v);
                        }
                    }
                    if (kStepNeg(kk)) A[mb] = neg3(A[mb]);      // (kk is a constant of the unrolled loop)
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    Frag3 Bf;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) Bf.p[pl] = *reinterpret_cast<const bf16x8*>(bsrc + ((kk * NB + nb) * 3 + pl) * 1024);
#pragma unroll
                    for (int mb = 0; mb < kMB; ++mb)
                        acc[mb][nb] = kStepNeg(kk) ? mma32x3_step<true>(A[mb], Bf, acc[mb][nb]) : mma32x3_step<false>(A[mb], Bf, acc[mb][nb]);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the next chunk's DMA pieces (and the A values) have landed
        __syncthreads();
    }

    // ---- epilogue: per 32 x 32 block, accumulator -> LDS tile [n][pixel] -> 128-byte rows of the output planes
    float* const tile = reinterpret_cast<float*>(s_b) + w * 32 * kTileLd;
    if constexpr (POOL) {
        // a block's tile holds 8 windows x 32 channels: lane (window j = lane & 7, channel lane >> 3 + 8 i) scans its window's four
        // columns 2 j, 2 j + 1, 16 + 2 j, 17 + 2 j by K9's rules (first maximum in scan order, a NaN wins, alive = !(m <= 0)); eight
        // lanes store 32 consecutive bytes of an output plane.  Where window j lies is known to the lanes that computed it: lane 2 j.
        const int j = lane & 7, cl = lane >> 3;
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            const bool wvalid = __shfl((int)valid[mb], 2 * j) != 0;
            const size_t wout = (size_t)(unsigned)__shfl((int)(unsigned)out_px[mb], 2 * j) |
                                ((size_t)(unsigned)__shfl((int)(unsigned)(out_px[mb] >> 32), 2 * j) << 32);
            [[maybe_unused]] size_t wpl = 0;
            if constexpr (OPL)
                wpl = (size_t)(unsigned)__shfl((int)(unsigned)out_pl[mb], 2 * j) | ((size_t)(unsigned)__shfl((int)(unsigned)(out_pl[mb] >> 32), 2 * j) << 32);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int n0 = (ng * NB + nb) * 32;
                if (n0 < a.Cout) {       // wave-uniform
#pragma unroll
                    for (int e = 0; e < 16; ++e) tile[(lane & 31) * kTileLd + acc_row_c(e, lane)] = acc[mb][nb][e];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own stores (no other wave touches this tile)
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = n0 + cl + 8 * i;
                        const bool live = wvalid && n < a.Cout;
                        const float bv = (pool_bias && live) ? pool_bias[n] : 0.0f;      // (a plain fp32 add, as K9's: no product to contract)
                        const float* const t = tile + (cl + 8 * i) * kTileLd + 2 * j;
                        const float v[4] = {t[0] + bv, t[1] + bv, t[16] + bv, t[17] + bv};
                        float m = v[0];
                        int k = 0;
#pragma unroll
                        for (int u = 1; u < 4; ++u)
                            if (v[u] > m || v[u] != v[u]) { m = v[u]; k = u; }
                        const bool alive = !(m <= 0.0f);
                        if (live) {
                            const size_t o = wout + (size_t)n * HWo;
                            a.z[o] = alive ? m : 0.0f;
                            pool_mask[o] = alive ? (uint8_t)k : (uint8_t)4;
                            if constexpr (OPL) {
                                // channel n is element cl of group n >> 3: the eight lanes of a window and group fill one 16-byte piece
                                unsigned p0, p1, p2;
                                split3(alive ? m : 0.0f, 0.0f, p0, p1, p2);
                                unsigned short* const d = out_planes + wpl + (size_t)((n >> 3) * 3) * HWo * 8 + cl;
                                d[0] = (unsigned short)p0;
                                d[(size_t)HWo * 8] = (unsigned short)p1;
                                d[(size_t)HWo * 16] = (unsigned short)p2;
                            }
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        return;
    }
#pragma unroll
    for (int mb = 0; mb < kMB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n0 = (ng * NB + nb) * 32;
            if (n0 < a.Cout) {       // wave-uniform
#pragma unroll
                for (int e = 0; e < 16; ++e) tile[(lane & 31) * kTileLd + acc_row_c(e, lane)] = acc[mb][nb][e];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own stores (no other wave touches this tile)
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int n = h + 2 * i;
                    if (valid[mb] && n0 + n < a.Cout) a.z[out_px[mb] + (size_t)(n0 + n) * HWo] = tile[n * kTileLd + (lane & 31)];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
        }
