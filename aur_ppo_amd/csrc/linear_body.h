// The body of every k_linear* product kernel (linear.hip), included INSIDE each kernel template: NB, MB, ROWS, GATE, GRAD and KTAIL are
// compile-time constants of the including kernel, `a` its product's LinArgs and `wg` the workgroup's index inside that product's grid
// (the paired kernels pick both from the net BEFORE this text, so nothing in here knows that there are two nets).  One text, so the
// builds cannot drift; compiled in place, so the kernels keep their names and their instruction streams (through a shared __device__
// function they kept neither).
// MB is the number of 32-row blocks per wave: kMB (k_linear, k_linear_tail: 256 rows x 32 NB columns per workgroup, NB up to 4), or 1
// (the small-M builds: 128 rows x 32 NB columns, NB <= 2, for the rollout's M of a few thousand rows, which k_linear spreads over an
// eighth of the chip).  A row's result depends on the row's values, the operand copy and the order of the k-steps alone -- split3 of
// the A values (an invalid row enters as 0), mma32x3_step<kStepNeg(ks)> per k-step in ks order, one rounded add per k-step, acc + bias
// and the tanh -- and none of that reads MB: the small tile's bits are k_linear's because they come from these very lines.
    static_assert(!(GRAD && KTAIL) && (GRAD || !GATE), "the input gradient's inner dimension is a hidden width");
    constexpr int kChunkBytes = kKC * NB * 3 * 1024;
    __shared__ __attribute__((aligned(16))) char s_b[2 * kChunkBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mbq = (int)(wg % (unsigned)a.n_mb), ng = (int)(wg / (unsigned)a.n_mb);
    const int h = lane >> 5;
    const int KS = KTAIL ? (a.K + 15) >> 4 : a.K >> 4;
    long long m0[MB];
    const float* row[MB];
    bool valid[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        m0[mb] = (((long long)mbq * 4 + w) * MB + mb) * 32;
        const long long m = m0[mb] + (lane & 31);
        valid[mb] = m < a.M;
        if (ROWS) row[mb] = a.x + (size_t)(valid[mb] ? a.rows[m] : 0) * a.K + 8 * h;
        else row[mb] = a.x + (size_t)(valid[mb] ? m : 0) * a.K + 8 * h;
    }
    const char* const wgrp = reinterpret_cast<const char*>(a.wop) + (size_t)(ng * NB) * KS * 3 * 1024;
    // A chunk is kKC * NB * 3 pieces of 1 KB (6 at NB = 1, 12 at NB = 2, 24 at NB = 4); wave w brings the pieces f = w, w + 4, ...: every
    // f has one wave, whatever the count (at 6 pieces waves 0 and 1 bring two, waves 2 and 3 one).
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
    f32x16c acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mb][nb][e] = 0.0f;
    auto load_a = [&](int ks, float4 (&v)[MB][2]) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            if constexpr (KTAIL) {
                const float* p = row[mb] + ks * 16;
                const int live = a.K - ks * 16 - 8 * h;        // how many of this lane's eight columns the row has
                float c[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) c[j] = j < live ? p[j] : 0.0f;
                v[mb][0] = float4{c[0], c[1], c[2], c[3]};
                v[mb][1] = float4{c[4], c[5], c[6], c[7]};
            } else {
                const float4* p = reinterpret_cast<const float4*>(row[mb] + ks * 16);
                v[mb][0] = p[0];
                v[mb][1] = p[1];
            }
        }
    };
    const int n_chunks = (KS + kKC - 1) / kKC;
    float4 abuf[2][MB][2];
    stage(0, 0);
    load_a(0, abuf[0]);
    // The DMA pieces are older than load_a's loads, and the vector memory counter retires in order: load_a is two 16-byte loads per row
    // block, so "all but the 2 MB youngest" is every DMA piece.  A tail lane issues up to eight dword loads per row block, fewer, or none.
    if constexpr (KTAIL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * MB) : "memory");
    __syncthreads();
    for (int kc = 0; kc < n_chunks; ++kc) {
        if (kc + 1 < n_chunks) stage(kc + 1, (kc + 1) & 1);
        const char* const bsrc = s_b + (kc & 1) * kChunkBytes + lane * 16;
#pragma unroll
        for (int kk = 0; kk < kKC; ++kk) {
            const int ks = kc * kKC + kk;
            if (ks < KS) {
                float4 (&cur)[MB][2] = abuf[kk];
                if (ks + 1 < KS) load_a(ks + 1, abuf[kk ^ 1]);
                // every k-step is summed from zero and added once, every other one negated (bf3_gemm.h::mma32x3_step): ks and kk have the
                // same parity, and the A values of a negated step are negated BEFORE the split (the split of -a is the negated split of a).
                // GRAD (the input gradient): the wave's two row blocks negate OPPOSITE steps.  Where the steps differ in size -- an
                // output gradient whose columns differ in scale: the cut follows the largest term of a step -- the cuts of neighbouring
                // steps do not cancel, and what is left has one sign for every row.  What consumes a gradient sums it over rows (the
                // weight and bias gradients of the layer below): with the other sign in the next block of 32 rows that sum cancels it.
                // The forward product keeps one pattern: a row's result must not depend on where the row stands (the rollout's
                // log-prob and value are the update's bit for bit).
                Frag3 A[MB];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const bool NEG = kStepNeg(kk + (GRAD ? mb : 0));     // (a constant once the loops are unrolled)
                    const float c[8] = {cur[mb][0].x, cur[mb][0].y, cur[mb][0].z, cur[mb][0].w, cur[mb][1].x, cur[mb][1].y, cur[mb][1].z, cur[mb][1].w};
                    unsigned p[4][3];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        split3(valid[mb] ? (NEG ? -c[2 * q] : c[2 * q]) : 0.0f, valid[mb] ? (NEG ? -c[2 * q + 1] : c[2 * q + 1]) : 0.0f, p[q][0],
                               p[q][1], p[q][2]);
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) {
                        const u32x4 v = {p[0][pl], p[1][pl], p[2][pl], p[3][pl]};
                        A[mb].p[pl] = __builtin_bit_cast(bf16x8, v);
                    }
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    Frag3 Bf;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) Bf.p[pl] = *reinterpret_cast<const bf16x8*>(bsrc + ((kk * NB + nb) * 3 + pl) * 1024);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb][nb] = kStepNeg(kk + (GRAD ? mb : 0)) ? mma32x3_step<true>(A[mb], Bf, acc[mb][nb])
                                                                     : mma32x3_step<false>(A[mb], Bf, acc[mb][nb]);
                }
            }
        }
        // everything this wave has in flight -- the next chunk's pieces and the next k-step's A values -- before the other waves read
        // the chunk and before this one's buffer is staged over
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = (ng * NB + nb) * 32 + (lane & 31);
            if (col < a.N) {
                const float bv = a.bias && col < a.n_bias ? a.bias[col] : 0.0f;      // (n_bias < N: the columns behind the layer's own add 0)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const long long r = m0[mb] + acc_row_c(e, lane);
                    float v = acc[mb][nb][e] + bv;
                    if (GATE) {
                        if (r < a.M) {
                            const float hv = a.h[(size_t)r * a.N + col];
                            a.y[(size_t)r * a.N + col] = v * (1.0f - hv * hv);
                        }
                        continue;
                    }
                    if (a.act == 1) v = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * v) + 1.0f);
                    if (r < a.M) a.y[(size_t)r * a.N + col] = v;
                }
            }
        }
