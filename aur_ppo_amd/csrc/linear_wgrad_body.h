// The body of k_linear_wgrad and k_linear_wgrad_tail (linear.hip), included INSIDE each of the kernel templates: ROWS, KTAIL and BIAS
// are compile-time constants of the including kernel, `a` its WgradArgs (see linear_body.h for why it is a text and not a function).
// BIAS: the workgroups of k-tile 0 also sum the dY pieces they fetch anyway over the slice's rows, per column, in fp64 (a thread's
// rows in ascending order, then the eight row groups in order), and leave one partial vector of N doubles per slice in a.bpart.
    __shared__ __attribute__((aligned(16))) char s_img[2 * 2 * 3 * kXPlane];      // [dY | X][64-column half][3 planes][32 rows x 128 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = (int)(blockIdx.x % (unsigned)(a.n_tiles_n * a.n_tiles_k)), s = (int)(blockIdx.x / (unsigned)(a.n_tiles_n * a.n_tiles_k));
    const int n0 = (tile / a.n_tiles_k) * 128, k0 = (tile % a.n_tiles_k) * 128;
    const long long m_lo = (long long)s * a.rows_per_slice;
    long long m_hi = m_lo + a.rows_per_slice;
    if (m_hi > a.M) m_hi = a.M;
    char* const imgA = s_img;                               // dY columns n0 .. n0 + 127
    char* const imgB = s_img + 2 * 3 * kXPlane;            // X columns k0 .. k0 + 127
    const int wn = w >> 1, wk = w & 1;                      // this wave's 64 x 64 quarter
    // staging: a chunk = 32 rows x 128 columns of each operand = 1024 float4 per operand, four per thread
    const int r_of = tid >> 5, c4 = (tid & 31) * 4;         // + 8 rows per further slot
    f32x16c acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    float pa[4][4], pb[4][4];
    [[maybe_unused]] double bs[4] = {0.0, 0.0, 0.0, 0.0};   // BIAS: this thread's column sums of dY columns n0 + c4 .. + 3
    [[maybe_unused]] const bool bias_wg = BIAS && k0 == 0;
    unsigned pok = 0u;               // bit u: dY piece u is real; bit 4 + u: X piece u (the zeroing waits until the chunk is staged)
    auto fetch = [&](long long m0) {
        pok = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long r = m0 + r_of + 8 * u;
            const bool okr = r < m_hi;
            const bool oka = okr && n0 + c4 < a.N, okb = okr && k0 + c4 < a.K;      // (N is a multiple of 4; K too unless KTAIL)
            const float4 va = *reinterpret_cast<const float4*>(a.dy + (oka ? (size_t)r * a.N + n0 + c4 : (size_t)0));
            const size_t xr = ROWS ? (size_t)(okb ? a.rows[r] : 0) : (size_t)r;
            float4 vb;
            if constexpr (KTAIL) {
                const float* const px = a.x + (okb ? xr * a.K + k0 + c4 : (size_t)0);
                vb.x = okb ? px[0] : 0.0f;
                vb.y = okb && k0 + c4 + 1 < a.K ? px[1] : 0.0f;
                vb.z = okb && k0 + c4 + 2 < a.K ? px[2] : 0.0f;
                vb.w = okb && k0 + c4 + 3 < a.K ? px[3] : 0.0f;
            } else vb = *reinterpret_cast<const float4*>(a.x + (okb ? xr * a.K + k0 + c4 : (size_t)0));
            pa[u][0] = va.x; pa[u][1] = va.y; pa[u][2] = va.z; pa[u][3] = va.w;
            pb[u][0] = vb.x; pb[u][1] = vb.y; pb[u][2] = vb.z; pb[u][3] = vb.w;
            pok |= (oka ? 1u : 0u) << u;
            pok |= (okb ? 1u : 0u) << (4 + u);
        }
    };
    fetch(m_lo);
    for (long long m0 = m_lo; m0 < m_hi; m0 += 32) {
        __syncthreads();                                    // the previous chunk's fragments have been read
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r_of + 8 * u;
            const bool oka = (pok >> u) & 1u, okb = (pok >> (4 + u)) & 1u;
            if constexpr (BIAS) {
                if (bias_wg && oka) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) bs[j] += (double)pa[u][j];
                }
            }
            store_x4(imgA + (c4 >> 6) * 3 * kXPlane, r, c4 & 63, oka ? pa[u][0] : 0.0f, oka ? pa[u][1] : 0.0f, oka ? pa[u][2] : 0.0f,
                     oka ? pa[u][3] : 0.0f);
            store_x4(imgB + (c4 >> 6) * 3 * kXPlane, r, c4 & 63, okb ? pb[u][0] : 0.0f, okb ? pb[u][1] : 0.0f, okb ? pb[u][2] : 0.0f,
                     okb ? pb[u][3] : 0.0f);
        }
        __syncthreads();
        if (m0 + 32 < m_hi) fetch(m0 + 32);                 // the next chunk's rows, behind this chunk's products
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const Frag3 A0 = x_cols(imgA + wn * 3 * kXPlane, ks, 0, lane), A1 = x_cols(imgA + wn * 3 * kXPlane, ks, 32, lane);
            const Frag3 B0 = x_cols(imgB + wk * 3 * kXPlane, ks, 0, lane), B1 = x_cols(imgB + wk * 3 * kXPlane, ks, 32, lane);
            // every k-step is summed from zero and added once, the second of a chunk negated (bf3_gemm.h::mma32x3_step)
            if (kStepNeg(ks)) {
                const Frag3 N0 = neg3(A0), N1 = neg3(A1);
                acc[0][0] = mma32x3_step<true>(N0, B0, acc[0][0]);
                acc[0][1] = mma32x3_step<true>(N0, B1, acc[0][1]);
                acc[1][0] = mma32x3_step<true>(N1, B0, acc[1][0]);
                acc[1][1] = mma32x3_step<true>(N1, B1, acc[1][1]);
            } else {
                acc[0][0] = mma32x3_step<false>(A0, B0, acc[0][0]);
                acc[0][1] = mma32x3_step<false>(A0, B1, acc[0][1]);
                acc[1][0] = mma32x3_step<false>(A1, B0, acc[1][0]);
                acc[1][1] = mma32x3_step<false>(A1, B1, acc[1][1]);
            }
        }
    }
    // C[m = dY column][n = X column]: the lane holds the X column, its registers the dY columns -- rows of `part` are contiguous over the lanes
    float* const out = a.part + (size_t)s * a.N * a.K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = k0 + wk * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = n0 + wn * 64 + i * 32 + acc_row_c(e, lane);
                if (row < a.N && col < a.K) out[(size_t)row * a.K + col] = acc[i][j][e];
            }
        }
    if constexpr (BIAS) {
        // the eight row groups' sums of a column meet in LDS (the images are done with) and thread n < 128 adds them in group order
        double* const s_bs = reinterpret_cast<double*>(s_img);           // [8 row groups][128 columns]
        __syncthreads();                                    // the last chunk's fragments have been read
        if (bias_wg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s_bs[r_of * 128 + c4 + j] = bs[j];
        }
        __syncthreads();
        if (bias_wg && tid < 128 && n0 + tid < a.N) {
            double t = 0.0;
#pragma unroll
            for (int g = 0; g < 8; ++g) t += s_bs[g * 128 + tid];
            a.bpart[(size_t)s * a.N + n0 + tid] = t;
        }
    }
