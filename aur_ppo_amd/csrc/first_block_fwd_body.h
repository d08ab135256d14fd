// The body of k_first_block_fwd (pool.hip), included INSIDE each of its two kernel templates, as conv3x3_body.h is: CI and OPL are
// compile-time constants of the including kernel, `out_planes` the OPL build's further argument (a null constant in the plain build) and
// AURPPO_FB_CHANNEL_LOOP the pragma in front of the loop over the 16 output channels (empty in the plain build, which keeps its
// instruction stream; `unroll` in the OPL build, whose packed planes are then indexed by constants and stay in registers).
//
// OPL (behind aurppo_first_block_planes_fwd_f32): beside y and the mask, the thread writes the planes of its pooled element's 16
// channels -- split3 of the very values it stores in y -- as two 16-byte pieces per plane (include/aurppo.h's layout: groups 2 cg and
// 2 cg + 1 of its image, pixel q).
    const int Ho = H >> 1, Wo = W >> 1;
    const int q = blockIdx.x * kFbThreads + threadIdx.x;
    const int cg = blockIdx.y, b = blockIdx.z;
    const bool live = q < Ho * Wo;
    const int ho = live ? q / Wo : 0, wo = live ? q - ho * Wo : 0;
    const float sv = state[b];
    // the 4x4 input patch of this pooled cell, per image channel (rows 2ho-1 .. 2ho+2, cols 2wo-1 .. 2wo+2), zero outside
    float p[CI][4][4];
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
        const float* op = obs + ((size_t)b * CI + ci) * H * W;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int h = 2 * ho - 1 + r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int ww = 2 * wo - 1 + c;
                const bool in = live && h >= 0 && h < H && ww >= 0 && ww < W;
                p[ci][r][c] = in ? op[(size_t)(in ? h : 0) * W + (in ? ww : 0)] : 0.0f;
            }
        }
    }
    // border classes of the four conv positions (rows 2ho, 2ho+1; cols 2wo, 2wo+1) as 0/1 factors: the state plane's
    // response is the sum of the channel's state taps that fall inside the image = all - border row - border column + corner
    const float ft = ho == 0 ? 1.0f : 0.0f, fb = 2 * ho + 1 == H - 1 ? 1.0f : 0.0f;
    const float fl = wo == 0 ? 1.0f : 0.0f, fr = 2 * wo + 1 == W - 1 ? 1.0f : 0.0f;
    [[maybe_unused]] unsigned pk[3][kFbCo / 2];      // OPL: plane pl of channels 2 i, 2 i + 1 in the halves of pk[pl][i]
    if constexpr (OPL) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int i = 0; i < kFbCo / 2; ++i) pk[pl][i] = 0u;
    }
    AURPPO_FB_CHANNEL_LOOP
    for (int cc = 0; cc < kFbCo; ++cc) {
        const int c = cg * kFbCo + cc;
        const float* wc = w + (size_t)c * (CI + 1) * 9;       // uniform address: scalar loads
        float acc[4];
        const float bv = bias ? bias[c] : 0.0f;
        const float* ts = wc + CI * 9;
        // state plane first, then the bias (the association of base_encoder.forward_split: (conv + state*plane) + bias)
        const float all = ((ts[0] + ts[1]) + (ts[2] + ts[3])) + ((ts[4] + ts[5]) + (ts[6] + ts[7])) + ts[8];
        const float r0 = ts[0] + ts[1] + ts[2], r2 = ts[6] + ts[7] + ts[8];
        const float c0 = ts[0] + ts[3] + ts[6], c2 = ts[2] + ts[5] + ts[8];
        const float pl[4] = {all - ft * r0 - fl * c0 + ft * fl * ts[0], all - ft * r0 - fr * c2 + ft * fr * ts[2],
                             all - fb * r2 - fl * c0 + fb * fl * ts[6], all - fb * r2 - fr * c2 + fb * fr * ts[8]};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = 0.0f;
#pragma unroll
        for (int ci = 0; ci < CI; ++ci)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float wv = wc[ci * 9 + kh * 3 + kw];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = fmaf(p[ci][(u >> 1) + kh][(u & 1) + kw], wv, acc[u]);
                }
        float m = 0.0f;
        int k = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float v = (acc[u] + sv * pl[u]) + bv;
            if (u == 0 || v > m || v != v) { m = v; k = u; }
        }
        const bool alive = !(m <= 0.0f);
        if (live) {
            const size_t o = (((size_t)b * Co + c) * Ho + ho) * Wo + wo;
            y[o] = alive ? m : 0.0f;
            mask[o] = alive ? (uint8_t)k : (uint8_t)4;
        }
        if constexpr (OPL) {
            unsigned p0, p1, p2;
            bf3::split3(alive ? m : 0.0f, 0.0f, p0, p1, p2);      // (the high halves are the planes of 0.0f: zero)
            pk[0][cc >> 1] |= p0 << (16 * (cc & 1));
            pk[1][cc >> 1] |= p1 << (16 * (cc & 1));
            pk[2][cc >> 1] |= p2 << (16 * (cc & 1));
        }
    }
    if constexpr (OPL) {
        if (live) {
            bf3::u32x4* const dst = reinterpret_cast<bf3::u32x4*>(out_planes) + ((size_t)b * (Co >> 3) + 2 * cg) * 3 * (Ho * Wo) + q;
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    dst[(size_t)(3 * g + pl) * (Ho * Wo)] = bf3::u32x4{pk[pl][4 * g], pk[pl][4 * g + 1], pk[pl][4 * g + 2], pk[pl][4 * g + 3]};
        }
    }
