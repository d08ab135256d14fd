// The tail of a fused MLP minibatch step (K7: mlp.hip, K7w: mlp_wide.hip), behind the step kernel's per-workgroup gradient slabs and
// loss partials:
//   * k_mlp_reduce_x4  -- K7's slab reduce: sums the slabs in fixed order (deterministic), folds the loss scalars, leaves the clip's
//                         partial sums, advances the Adam step count and forms its bias corrections;
//   * k_mlp_reduce<1,2> -- K7w's: the same sums on 4-byte loads over slabs of stride n_params, up to 256 or 512 of them;
//   * k_adam_chain     -- clip + Adam, refreshes the operand-order copies of every family (refresh_operand_copies), prepares the next
//                         minibatch's statistics;
// and their host side: launch_adam_chain (every launch of k_adam_chain) and launch_mlp_tail (reduce, then the optimizer launch).
// No `#pragma clang fp contract(fast)` here: the Adam arithmetic is held to fp64 references with contraction off.
#include <stdlib.h>

#include "adam_math.h"
#include "bf16x3.h"
#include "mlp_tail.h"

using namespace aurppo_mlp;

namespace {

// The nine scalars of a minibatch from its six loss sums (r: pg, vl, ent, old KL, KL, clip fraction) and advantage statistics
__device__ __forceinline__ void write_loss_scalars(const double* r, const PpoHyper& h, double adv_mean, double adv_std,
                                                   float* __restrict__ out_scalars) {
    const double M = (double)h.M;
    const float pg = (float)(r[0] / M), vl = 0.5f * (float)(r[1] / M), ent = (float)(r[2] / M);
    out_scalars[AURPPO_S_PG] = pg;
    out_scalars[AURPPO_S_VL] = vl;
    out_scalars[AURPPO_S_ENT] = ent;
    out_scalars[AURPPO_S_OLD_KL] = (float)(r[3] / M);
    out_scalars[AURPPO_S_KL] = (float)(r[4] / M);
    out_scalars[AURPPO_S_CLIPFRAC] = (float)(r[5] / M);
    out_scalars[AURPPO_S_LOSS] = (pg - h.ent_coef * ent) + vl * h.vf_coef;
    out_scalars[AURPPO_S_ADV_MEAN] = (float)adv_mean;
    out_scalars[AURPPO_S_ADV_STD] = (float)adv_std;
}

// ---- The slab reduce: grads[p] = sum over slabs in a fixed order (deterministic); workgroup 0 also folds the loss scalars.
// A workgroup owns 64 parameters and 16 slab groups; group grp takes the rows b = grp (mod 16), 16 of them (per half) in flight per
// thread, and the groups are combined through LDS in order.  sq_part != nullptr (chained minibatch step): also the clip's partial sums
// of squares, one per workgroup; step_dev != nullptr: the Adam step count is advanced and the tile counters of the next step launch
// are cleared.  Two kernels, which differ in how a thread fetches its rows (4-byte loads over slabs of stride n_params, 1024 threads;
// 16-byte loads over slabs of stride slab_stride(n_params), 256 threads: DESIGN 4.3, round 5) and share everything behind the fetch:
// the four passages below, each expanded in place where the call stands.  (With them both kernels keep the registers, LDS and launch
// times of the written-out text; the instruction streams differ from it in operand order and by one or two scalar instructions:
// profiles/refactor_mlp_tail.txt.)
constexpr int kRedGroups = 16;

// One parameter's sum over a group's 16 rows, x(j) = row grp + 16 j: ((x0 + x4) + x8) + x12 per quarter, (a0 + a1) + (a2 + a3)
template <class X>
__device__ __forceinline__ float row_tree(X x) {
    float a4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a4[k] = ((x(k) + x(k + 4)) + x(k + 8)) + x(k + 12);
    return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}

// stepper: this is the one thread that advances the Adam step count (step_dev && thread 0 of workgroup 0); t_new: the step this
// minibatch is.  Adam's bias corrections for the optimizer launch that follows, formed while the slab rows are on their way:
__device__ __forceinline__ void bias_corrections(bool stepper, float t_new, double beta1, double beta2, double* __restrict__ bc_out) {
    if (stepper && bc_out) {
        bc_out[0] = 1.0 - pow(beta1, (double)t_new);
        bc_out[1] = 1.0 - pow(beta2, (double)t_new);
    }
}

// Wave 0, lane pi of parameter p = 64 blockIdx.x + pi: the 16 groups' sums folded 0 -> 15 from 0.0 into grads[p], the clip's partial
// sum of the workgroup's 64 squares, and the step advance with the two counter words cleared
__device__ __forceinline__ void fold_groups(const float (&s_part)[kRedGroups][64], int pi, int p, int n_params,
                                            float* __restrict__ grads, double* __restrict__ sq_part, bool stepper, float t_new,
                                            float* __restrict__ step_dev, unsigned* __restrict__ tile_counter) {
    float t = 0.0f;
    if (p < n_params) {
#pragma unroll
        for (int g = 0; g < kRedGroups; ++g) t += s_part[g][pi];
        grads[p] = t;
    }
    if (sq_part) {
        const double q = wave_sum((double)t * (double)t);
        if (pi == 0) sq_part[blockIdx.x] = q;
    }
    if (stepper) {
        *step_dev = t_new;   // the Adam kernel (a later launch) reads the new step count
        tile_counter[0] = 0u;
        tile_counter[1] = 0u;
    }
}

// The loss fold of workgroup 0, one wave per quantity q: lane l has added the partials of rows l, l + 64, ... from 0.0 into s; the
// shuffle reduce leaves the quantity's sum in r[q] ...
__device__ __forceinline__ void loss_fold_wave(double s, int q, int l, double* r) {
    s = wave_sum(s);
    if (l == 0) r[q] = s;
}
// ... and behind the barrier one thread writes the nine scalars (adv: the advantages' mean and standard deviation)
__device__ __forceinline__ void loss_fold_finish(bool folder, const double* r, const PpoHyper& h, const double* adv,
                                                 float* __restrict__ out_scalars) {
    __syncthreads();
    if (folder) write_loss_scalars(r, h, adv[0], adv[1], out_scalars);
}

template <int HALVES>   // 16 slab rows per thread and half: 256 slabs (K7w) or 512 (K7w with two workgroups per CU)
__global__ __launch_bounds__(1024) void k_mlp_reduce(const float* __restrict__ slabs, const double* __restrict__ loss_part,
                                                     int n_slabs, int n_params, PpoHyper h, float* __restrict__ grads,
                                                     float* __restrict__ out_scalars, double* __restrict__ sq_part,
                                                     float* __restrict__ step_dev, unsigned* __restrict__ tile_counter,
                                                     double beta1, double beta2, double* __restrict__ bc_out) {
    __shared__ float s_part[kRedGroups][64];
    const int pi = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + pi;
    const bool stepper = step_dev && threadIdx.x == 0 && blockIdx.x == 0;
    const float t_new = stepper ? *step_dev + 1.0f : 0.0f;      // the Adam step this minibatch is
    float acc = 0.0f;
    if (p < n_params) {
        // n_slabs <= kMaxGrid = 16 groups x 16: a thread's rows are all fetched before the first add (one memory round
        // trip, not four); rows past n_slabs read as zero; the order of the adds is fixed
        static_assert(kMaxGrid <= 16 * kRedGroups, "k_mlp_reduce: 16 rows per thread cover the grid");
        float x[16 * HALVES];
#pragma unroll
        for (int j = 0; j < 16 * HALVES; ++j) {
            const int b = grp + j * kRedGroups;
            x[j] = b < n_slabs ? slabs[(size_t)b * n_params + p] : 0.0f;
        }
        bias_corrections(stepper, t_new, beta1, beta2, bc_out);
#pragma unroll
        for (int h = 0; h < HALVES; ++h) {
            const float ah = row_tree([&](int k) { return x[16 * h + k]; });
            acc = h == 0 ? ah : acc + ah;
        }
    }
    s_part[grp][pi] = acc;
    __syncthreads();
    if (grp == 0) fold_groups(s_part, pi, p, n_params, grads, sq_part, stepper, t_new, step_dev, tile_counter);   // wave 0
    __shared__ double r[6];
    if (blockIdx.x == 0 && threadIdx.x < 6 * kWave) {
        // lanes stride over the workgroups' partials
        const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
        double s = 0.0;
        for (int b = l; b < n_slabs; b += kWave) s += loss_part[(size_t)b * 8 + q];
        loss_fold_wave(s, q, l, r);
    }
    loss_fold_finish(blockIdx.x == 0 && threadIdx.x == 0, r, h, loss_part + 6, out_scalars);
}

// K7's slab reduce (slabs of slab_stride floats, n_slabs <= kMaxGrid) on 16-byte loads: a thread holds FOUR consecutive parameters of
// its group's 16 rows (16 x 16 B in flight per lane, one wave-instruction = four 256-B row segments) where k_mlp_reduce<1> holds one of
// them in 4-byte loads, which moved the 17 MB of slabs at a third of what the chip streams.  The loss partials are fetched ahead too
// (two quantities for the first two waves).
__global__ __launch_bounds__(256) void k_mlp_reduce_x4(const float* __restrict__ slabs, const double* __restrict__ loss_part,
                                                       int n_slabs, int n_params, PpoHyper h, float* __restrict__ grads,
                                                       float* __restrict__ out_scalars, double* __restrict__ sq_part,
                                                       float* __restrict__ step_dev, unsigned* __restrict__ tile_counter,
                                                       double beta1, double beta2, double* __restrict__ bc_out) {
    __shared__ __attribute__((aligned(16))) float s_part[kRedGroups][64];
    const int qi = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int p0 = blockIdx.x * 64 + 4 * qi;
    const int ns = slab_stride(n_params);
    const bool stepper = step_dev && threadIdx.x == 0 && blockIdx.x == 0;
    static_assert(kMaxGrid <= 16 * kRedGroups, "k_mlp_reduce_x4: 16 rows per thread cover the grid");
    float4 x[16];
    if (p0 + 3 < n_params) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int b = grp + j * kRedGroups;
            x[j] = b < n_slabs ? *reinterpret_cast<const float4*>(slabs + (size_t)b * ns + p0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {   // the bucket's last, partial quad (or none): parameters past n_params read as zero, the stride's padding is not read
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int b = grp + j * kRedGroups;
            const float* r = slabs + (size_t)b * ns + p0;
            const bool ok = b < n_slabs;
            x[j] = make_float4(ok && p0 + 0 < n_params ? r[0] : 0.f, ok && p0 + 1 < n_params ? r[1] : 0.f,
                               ok && p0 + 2 < n_params ? r[2] : 0.f, ok && p0 + 3 < n_params ? r[3] : 0.f);
        }
    }
    // workgroup 0 also folds the loss partials: they are fetched here, behind the slab rows, so that its fold costs no memory
    // round trip of its own after the gradient's (waves 0 and 1 hold quantities w and w + 4, waves 2 and 3 quantity w; what
    // lies past n_slabs or names no quantity is fetched from a valid row and not added)
    static_assert(kMaxGrid <= 4 * kWave, "k_mlp_reduce_x4: four partials per lane cover the grid");
    const int lw = threadIdx.x >> 6, ll = threadIdx.x & 63;
    double lq[2][4];
    double adv[2] = {0.0, 0.0};
    const bool folder = blockIdx.x == 0 && threadIdx.x == 0;
    if (blockIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = lw + 4 * u < 6 ? lw + 4 * u : 0, b = ll + k * kWave < n_slabs ? ll + k * kWave : 0;
                lq[u][k] = loss_part[(size_t)b * 8 + q];
            }
        adv[0] = loss_part[6];
        adv[1] = loss_part[7];
    }
    const float t_new = stepper ? *step_dev + 1.0f : 0.0f;      // the Adam step this minibatch is
    bias_corrections(stepper, t_new, beta1, beta2, bc_out);
    float4 acc;
    acc.x = row_tree([&](int k) { return x[k].x; });
    acc.y = row_tree([&](int k) { return x[k].y; });
    acc.z = row_tree([&](int k) { return x[k].z; });
    acc.w = row_tree([&](int k) { return x[k].w; });
    // (k_mlp_reduce leaves 0 for a parameter past n_params; here such a parameter's rows read as zero: the same)
    *reinterpret_cast<float4*>(&s_part[grp][4 * qi]) = acc;
    __syncthreads();
    if (threadIdx.x < 64)   // wave 0
        fold_groups(s_part, threadIdx.x, blockIdx.x * 64 + threadIdx.x, n_params, grads, sq_part, stepper, t_new, step_dev, tile_counter);
    __shared__ double r[6];
    if (blockIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = lw + 4 * u;
            if (q < 6) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ll + k * kWave < n_slabs) s += lq[u][k];
                loss_fold_wave(s, q, ll, r);
            }
        }
    }
    loss_fold_finish(folder, r, h, adv, out_scalars);
}

// bucket element i has just become pn: drop it wherever the weight appears as an operand (mlp_common.h's index functions say where)
__device__ __forceinline__ void refresh_operand_copies(const OperandCopies& oc, int i, float pn) {
    if (oc.wide.wop) {
        // K7w: forward copy of every hidden layer, backward copy of layers >= 1
        const aurppo_mlp::WideCopies& wc = oc.wide;
        for (int n = 0; n < 2; ++n)
            for (int l = 0; l < wc.NL; ++l) {
                const int in_dim = l == 0 ? wc.D : wc.Hd;
                const int e = i - wc.w[n][l];
                if (e < 0 || e >= wc.Hd * in_dim) continue;
                const int row = e / in_dim, col = e - row * in_dim;
                if (wc.wop3) {      // k_mlpw3_step's copies: the bf16 planes of the new value
                    unsigned p0, p1, p2;
                    bf3::split3(pn, 0.0f, p0, p1, p2);
                    for (int dir = 0; dir < (l > 0 ? 2 : 1); ++dir) {
                        const int at = op3_index(n, l, dir, row, col);
                        wc.wop3[at] = (unsigned short)p0;
                        wc.wop3[at + kOp3Plane] = (unsigned short)p1;
                        wc.wop3[at + 2 * kOp3Plane] = (unsigned short)p2;
                    }
                    continue;
                }
                wc.wop[op_index(n, l, 0, row, col)] = pn;
                if (l > 0) wc.wop[op_index(n, l, 1, row, col)] = pn;
            }
        return;
    }
    const int D = oc.D;
    const int ea = i - oc.w1_actor, ec = i - oc.w1_critic;
    const int e = (ea >= 0 && ea < H * D) ? ea : ((ec >= 0 && ec < H * D) ? ec : -1);
    if (e >= 0 && oc.w1op) {
        const int net = (ea >= 0 && ea < H * D) ? 0 : 1;
        const int row = e / D, k = e - row * D;
        oc.w1op[w1op_index(net, row, k)] = pn;
    }
    if (oc.wop3) {      // k_mlp_step3's copies: the bf16 planes of the new value wherever the weight appears as an operand
        const int e2a = i - oc.w2_actor, e2c = i - oc.w2_critic;
        const int e2 = (e2a >= 0 && e2a < H * H) ? e2a : ((e2c >= 0 && e2c < H * H) ? e2c : -1);
        if (e >= 0 || e2 >= 0) {
            const bool is_w2 = e < 0;
            const int net = is_w2 ? ((e2a >= 0 && e2a < H * H) ? 0 : 1) : ((ea >= 0 && ea < H * D) ? 0 : 1);
            const int row = is_w2 ? e2 / H : e / D;
            const int col = is_w2 ? e2 % H : e - (e / D) * D;
            int at[2];
            const int n_at = bf3::wop3_places(net, is_w2 ? 1 : 0, row, col, at);
            unsigned p0, p1, p2;
            bf3::split3(pn, 0.0f, p0, p1, p2);
            for (int q = 0; q < n_at; ++q) {
                oc.wop3[at[q]] = (unsigned short)p0;
                oc.wop3[at[q] + bf3::kWopBlock] = (unsigned short)p1;
                oc.wop3[at[q] + 2 * bf3::kWopBlock] = (unsigned short)p2;
            }
        }
    }
}

// Workgroups of k_adam_chain that update the bucket: one parameter per thread up to 128 workgroups.  The clip preamble is the
// same in every workgroup, and what a thread does per parameter -- Adam, the operand-copy refresh with its run-time division,
// bf16 split and scattered stores -- is one dependent chain: four per thread on 17 workgroups took 8.5 us per K7 minibatch,
// one per thread on 67 takes 6.4.  The result does not depend on it (the update is per element).
int adam_update_blocks(int n) {
    const int nb = (n + kThreads - 1) / kThreads;
    return nb < 128 ? nb : 128;
}

// Chained minibatch step, third launch: global-norm clip + Adam over the bucket (K6b's arithmetic); the W1
// elements it has just updated are dropped into the operand-order copy the next K7 launch streams; and the
// workgroups past `nb_upd` form the next minibatch's advantage partial sums -- so nothing is left to prepare
// before that launch.
__global__ __launch_bounds__(kThreads) void k_adam_chain(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, int n, const double* __restrict__ part,
                                                         int n_part, float max_norm, const float* __restrict__ lr_dev,
                                                         const float* __restrict__ step, double beta1, double beta2,
                                                         double eps, float* __restrict__ out_norm, float gscale, int nb_upd,
                                                         OperandCopies oc, const float4* __restrict__ rec, int rec_stride,
                                                         const int32_t* __restrict__ next_idx, int next_M,
                                                         double (*__restrict__ stats)[2], const double* __restrict__ bc) {
    __shared__ double sc[2][kThreads / kWave];
    __shared__ float s_coef;
    if ((int)blockIdx.x < nb_upd) {
        __shared__ double s_own;
        // a thread's first elements (up to four: one at the bucket sizes of K7, adam_update_blocks) are fetched before the
        // clip preamble, whose partial sums, block reductions and pow() calls they then overlap
        constexpr int kPre = 4;
        float p0[kPre], g0[kPre], m0[kPre], v0[kPre];
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int i = (blockIdx.x + k * nb_upd) * kThreads + threadIdx.x;
            const bool ok = i < n;
            p0[k] = ok ? p[i] : 0.0f;
            g0[k] = ok ? g[i] : 0.0f;
            m0[k] = ok ? m[i] : 0.0f;
            v0[k] = ok ? v[i] : 0.0f;
        }
        if (!part) {
            // no partial sums were left by k_mlp_reduce (the gradient went through an all-reduce since): every
            // workgroup forms the norm of the scaled gradient itself, in the same order -- 17 k floats, L2-resident
            // 16-B loads, all of a thread's in flight before the first add (n = 17 k: 17 per thread)
            double q = 0.0;
            const int n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? n / 4 : 0;
            const float4* g4 = reinterpret_cast<const float4*>(g);
            constexpr int kU = 8;
            for (int i0 = threadIdx.x; i0 < n4; i0 += kU * kThreads) {
                float4 x[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const int i = i0 + u * kThreads;
                    x[u] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const double a0 = (double)(x[u].x * gscale), a1 = (double)(x[u].y * gscale);
                    const double a2 = (double)(x[u].z * gscale), a3 = (double)(x[u].w * gscale);
                    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                }
            }
            for (int i = 4 * n4 + threadIdx.x; i < n; i += kThreads) {
                const double x = (double)(g[i] * gscale);
                q += x * x;
            }
            const double t = block_sum<kThreads / kWave>(q, sc[1]);
            if (threadIdx.x == 0) s_own = t;
            __syncthreads();
        }
        AdamScalars a = adam_scalars<kThreads / kWave>(part ? part : &s_own, part ? n_part : 1, max_norm, lr_dev, step, beta1,
                                                       beta2, eps, out_norm, blockIdx.x == 0, sc[0], &s_coef, bc);
        a.gscale = gscale;
        int k = 0;
        for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += nb_upd * kThreads, ++k) {
            // in-kernel norm: g is still being read by the other workgroups, so the clipped value is not stored back
            float pn;
            if (k < kPre) {
                float pk = p0[0], gk = g0[0], mk = m0[0], vk = v0[0];
#pragma unroll
                for (int j = 1; j < kPre; ++j)
                    if (k == j) { pk = p0[j]; gk = g0[j]; mk = m0[j]; vk = v0[j]; }
                pn = adam_update_pre(p, g, m, v, i, pk, gk, mk, vk, a, part != nullptr);
            } else {
                pn = adam_update(p, g, m, v, i, true, a, part != nullptr);
            }
            refresh_operand_copies(oc, i, pn);
        }
    } else {
        const int nsb = gridDim.x - nb_upd, b = blockIdx.x - nb_upd;
        double s = 0.0, q = 0.0;
        adv_partial_sums(rec, rec_stride, next_idx, next_M, b * kThreads + threadIdx.x, nsb * kThreads, s, q);
        const double bs = block_sum<kThreads / kWave>(s, sc[0]);
        const double bq = block_sum<kThreads / kWave>(q, sc[1]);
        if (threadIdx.x == 0) {
            stats[b][0] = bs;
            stats[b][1] = bq;
        }
    }
}

}  // namespace

OperandCopies aurppo_mlp::operand_copies(int n_params, const MlpLayout* L, int D, float* w1op, unsigned short* wop3, const WideCopies* wide) {
    OperandCopies oc = {L ? L->w1[0] : n_params, L ? L->w1[1] : n_params, D, w1op, L ? L->w2[0] : n_params, L ? L->w2[1] : n_params, wop3, {}};
    oc.wide.wop = nullptr;
    if (wide) oc.wide = *wide;
    return oc;
}

int aurppo_mlp::launch_adam_chain(const AdamLaunch& a, hipStream_t s) {
    const int nb_upd = adam_update_blocks(a.n_params);
    const int nsb = (a.next_idx && a.stats) ? stat_blocks_for(a.next_M) : 0;
    hipLaunchKernelGGL(k_adam_chain, dim3(nb_upd + nsb), dim3(kThreads), 0, s, a.params, a.grads, a.exp_avg, a.exp_avg_sq, a.n_params,
                       a.sq_part, a.n_part, (float)a.max_norm, a.lr_dev, a.step_dev, a.beta1, a.beta2, a.eps, a.out_norm, a.gscale, nb_upd,
                       a.copies, a.rec, a.rec_stride, nsb ? a.next_idx : (const int32_t*)nullptr, nsb ? a.next_M : 0,
                       reinterpret_cast<double (*)[2]>(a.stats), a.bc);
    AURPPO_LAUNCH_CHECK("k_adam_chain");
    return AURPPO_OK;
}

// grads[p] = fixed-order sum over n_slabs slabs, loss scalars folded.  sq_part / step_dev != nullptr: also leave the clip's partial sums
// of squares (one per 64 parameters) and advance the Adam step count; bc_out: {1 - beta1^t, 1 - beta2^t} for the optimizer launch.
static int launch_mlp_reduce(const TailWork& w, hipStream_t s, double* sq_part, float* step_dev, double beta1, double beta2, double* bc_out) {
    // (the reduce clears the step kernel's tile counters when it advances the step: the caller names words it may clear)
    AURPPO_REQUIRE(!step_dev || w.counters, AURPPO_EINVAL, "launch_mlp_reduce: step_dev without a scratch counter");
    // (k_mlp_reduce_x4 covers kMaxGrid slabs, k_mlp_reduce<2> twice as many)
    AURPPO_REQUIRE(w.n_slabs >= 1 && w.n_slabs <= (w.slab_strided ? 1 : 2) * kMaxGrid, AURPPO_ESHAPE, "launch_mlp_reduce: n_slabs=%d", w.n_slabs);
    const dim3 grid((w.n_params + 63) / 64);
    if (w.slab_strided) {
        hipLaunchKernelGGL(k_mlp_reduce_x4, grid, dim3(256), 0, s, w.slabs, w.loss_part, w.n_slabs, w.n_params, w.h, w.grads, w.out_scalars,
                           sq_part, step_dev, w.counters, beta1, beta2, bc_out);
        AURPPO_LAUNCH_CHECK("k_mlp_reduce_x4");
        return AURPPO_OK;
    }
    if (w.n_slabs <= kMaxGrid)
        hipLaunchKernelGGL(k_mlp_reduce<1>, grid, dim3(1024), 0, s, w.slabs, w.loss_part, w.n_slabs, w.n_params, w.h, w.grads, w.out_scalars,
                           sq_part, step_dev, w.counters, beta1, beta2, bc_out);
    else
        hipLaunchKernelGGL(k_mlp_reduce<2>, grid, dim3(1024), 0, s, w.slabs, w.loss_part, w.n_slabs, w.n_params, w.h, w.grads, w.out_scalars,
                           sq_part, step_dev, w.counters, beta1, beta2, bc_out);
    AURPPO_LAUNCH_CHECK("k_mlp_reduce");
    return AURPPO_OK;
}

int aurppo_mlp::launch_mlp_tail(const TailWork& w, const MlpTail* tail, hipStream_t s) {
    const bool optimize = tail && !tail->grad_only;
    // (words 8..11 of the counter block: Adam's two bias corrections, formed by the reduce for the optimizer launch behind it)
    double* const bc = optimize ? reinterpret_cast<double*>(w.counters + 8) : nullptr;
    const int rc = launch_mlp_reduce(w, s, optimize ? w.sq_part : nullptr, tail ? tail->step_dev : nullptr, optimize ? tail->beta1 : 0.0,
                                     optimize ? tail->beta2 : 0.0, bc);
    if (rc != AURPPO_OK || !optimize) return rc;
    AdamLaunch a = {};
    a.params = tail->params_rw; a.grads = w.grads; a.exp_avg = tail->exp_avg; a.exp_avg_sq = tail->exp_avg_sq; a.n_params = w.n_params;
    a.sq_part = w.sq_part; a.n_part = (w.n_params + 63) / 64; a.gscale = 1.0f;
    a.max_norm = tail->max_norm; a.lr_dev = tail->lr_dev; a.step_dev = tail->step_dev;
    a.beta1 = tail->beta1; a.beta2 = tail->beta2; a.eps = tail->eps; a.out_norm = tail->out_norm;
    a.copies = w.copies;
    a.rec = w.rec; a.rec_stride = w.rec_stride; a.next_idx = tail->next_idx; a.next_M = tail->next_M; a.stats = w.stats;
    a.bc = bc;
    return launch_adam_chain(a, s);
}
