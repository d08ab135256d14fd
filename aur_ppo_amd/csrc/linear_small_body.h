// The body of k_linear_small / k_linear_small_tail and of their paired forms k_linear_pair / k_linear_pair_tail (linear.hip), included
// INSIDE each kernel template: NB (1 or 2) and KTAIL are compile-time constants of the including kernel, `a` its product's LinArgs
// (x, wop, y, bias, M, K, N, n_mb, act; rows and h are not read) and `wg` the workgroup's index inside that product's grid -- the
// paired kernels pick both from the net BEFORE this text, so nothing in here knows that there are two nets.
// The forward product of linear_body.h on a smaller tile: four waves, ONE 32-row block per wave, NB <= 2 column blocks -- 128 rows x
// 32 NB columns where k_linear takes 256 x 128 -- for the rollout's M of a few thousand rows, which k_linear spreads over an eighth
// of the chip.  A row's result depends on the row's values, the operand copy and the order of the k-steps alone, and those are
// linear_body.h's: split3 of the A values (an invalid row enters as 0), mma32x3_step<kStepNeg(ks)> per k-step in ks order (the forward
// pattern, no GRAD alternation), one rounded add per k-step, acc + bias and the same tanh.  So the bits are k_linear's.
    constexpr int kChunkBytes = kKC * NB * 3 * 1024;
    __shared__ __attribute__((aligned(16))) char s_b[2 * kChunkBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mbq = (int)(wg % (unsigned)a.n_mb), ng = (int)(wg / (unsigned)a.n_mb);
    const int h = lane >> 5;
    const int KS = KTAIL ? (a.K + 15) >> 4 : a.K >> 4;
    const long long m0 = ((long long)mbq * 4 + w) * 32;
    const bool valid = m0 + (lane & 31) < a.M;
    const float* const row = a.x + (size_t)(valid ? m0 + (lane & 31) : 0) * a.K + 8 * h;
    const char* const wgrp = reinterpret_cast<const char*>(a.wop) + (size_t)(ng * NB) * KS * 3 * 1024;
    // A chunk is kKC * NB * 3 pieces of 1 KB (6 at NB = 1, 12 at NB = 2); wave w brings the pieces f = w, w + 4, ...: every f has one
    // wave, whatever the count (at 6 pieces waves 0 and 1 bring two, waves 2 and 3 one).
    auto stage = [&](int kc, int buf) {
        char* const dst = s_b + buf * kChunkBytes;
#pragma unroll
        for (int f = 0; f < kKC * NB * 3; ++f) {
            if ((f & 3) != w) continue;
            const int pl = f % 3, nb = (f / 3) % NB, kk = f / (3 * NB);
            const int ks = kc * kKC + kk;
            if (ks < KS) dma16(wgrp + ((size_t)(nb * KS + ks) * 3 + pl) * 1024 + lane * 16, dst + f * 1024);
        }
    };
    f32x16c acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nb][e] = 0.0f;
    auto load_a = [&](int ks, float4 (&v)[2]) {
        if constexpr (KTAIL) {
            const float* p = row + ks * 16;
            const int live = a.K - ks * 16 - 8 * h;        // how many of this lane's eight columns the row has
            float c[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = j < live ? p[j] : 0.0f;
            v[0] = float4{c[0], c[1], c[2], c[3]};
            v[1] = float4{c[4], c[5], c[6], c[7]};
        } else {
            const float4* p = reinterpret_cast<const float4*>(row + ks * 16);
            v[0] = p[0];
            v[1] = p[1];
        }
    };
    const int n_chunks = (KS + kKC - 1) / kKC;
    float4 abuf[2][2];
    stage(0, 0);
    load_a(0, abuf[0]);
    // The DMA pieces are older than load_a's loads, and the vector memory counter retires in order: with one row block load_a is TWO
    // 16-byte loads, so "all but the two youngest" is every DMA piece.  A tail lane issues up to eight dword loads, fewer, or none.
    if constexpr (KTAIL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    __syncthreads();
    for (int kc = 0; kc < n_chunks; ++kc) {
        if (kc + 1 < n_chunks) stage(kc + 1, (kc + 1) & 1);
        const char* const bsrc = s_b + (kc & 1) * kChunkBytes + lane * 16;
#pragma unroll
        for (int kk = 0; kk < kKC; ++kk) {
            const int ks = kc * kKC + kk;
            if (ks < KS) {
                float4 (&cur)[2] = abuf[kk];
                if (ks + 1 < KS) load_a(ks + 1, abuf[kk ^ 1]);
                const bool NEG = kStepNeg(kk);          // ks and kk have the same parity (kKC is even); a constant once unrolled
                const float c[8] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w};
                unsigned p[4][3];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    split3(valid ? (NEG ? -c[2 * q] : c[2 * q]) : 0.0f, valid ? (NEG ? -c[2 * q + 1] : c[2 * q + 1]) : 0.0f, p[q][0], p[q][1],
                           p[q][2]);
                Frag3 A;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const u32x4 v = {p[0][pl], p[1][pl], p[2][pl], p[3][pl]};
                    A.p[pl] = __builtin_bit_cast(bf16x8, v);
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    Frag3 Bf;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) Bf.p[pl] = *reinterpret_cast<const bf16x8*>(bsrc + ((kk * NB + nb) * 3 + pl) * 1024);
                    acc[nb] = NEG ? mma32x3_step<true>(A, Bf, acc[nb]) : mma32x3_step<false>(A, Bf, acc[nb]);
                }
            }
        }
        // everything this wave has in flight -- the next chunk's pieces and the next k-step's A values -- before the other waves read
        // the chunk and before this one's buffer is staged over
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = (ng * NB + nb) * 32 + (lane & 31);
        if (col < a.N) {
            const float bv = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long r = m0 + acc_row_c(e, lane);
                float v = acc[nb][e] + bv;
                if (a.act == 1) v = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * v) + 1.0f);
                if (r < a.M) a.y[(size_t)r * a.N + col] = v;
            }
        }
    }
