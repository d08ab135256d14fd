// The layered steps for the MLP policies the fused K7 / K7w steps do not cover (hidden_dim > 128 or more than 128 state floats): host
// code only, no kernel of its own.  The hidden layers run a layer at a time on linear.hip's products, the heads on head.hip's K13 (the
// update step, aurppo_mlp_layered_step_f32 / _minibatch_f32) and K14 (the rollout step, aurppo_mlp_layered_prep_f32 + _act_f32).
//
// Any hidden width (the aurppo_mlp_layered_anyh_* entries): a policy of width `hidden` runs as the policy of width
// Hp = 32 ceil(hidden / 32) whose extra weights and biases are zero -- entries that do not exist in the bucket and are never written.
// That is exact: a pad unit's pre-activation is 0, 1 - 2 / (e^0 + 1) is exactly 0, its outgoing weights are zero planes, gz of a pad
// column is 0 * (1 - 0), and every sum over a hidden axis gains exact zeros and nothing else.  So the activation planes are (M, Hp),
// from layer 1 on every product sees K = N = Hp on its aligned build, and the padded shape meets the bucket in four places only: the
// operand copies (k_linear_prep_pad), the bias read (LinArgs::n_bias), the weight gradients' fold (k_fold_slices_pad) and K13 / K14's
// head rows (HeadArgs::Hr).  Every function below takes `hidden` and forms Hp itself; at a multiple of 32 the two are equal and each
// call is the one it always was.  The old entries refuse the other widths before they come here (`anyh` false).
//
// Up to 32 actions (the aurppo_mlp_layered_wa_* entries, which take any hidden width too): nothing below the heads sees A, so the action
// limit `max_a` (16 | 32) travels next to `anyh` into the shape check and K13's run, and head.hip picks the kernels' NA = 32 builds for
// A in 17 .. 32.  The operand copies and the rollout workspace do not depend on A: the wa act entries take the anyh prep's buffer.
#include "mlp_common.h"

namespace {

bool layered_width_ok(int hidden, bool anyh) { return hidden >= (anyh ? 1 : 32) && hidden <= 1024 && (anyh || hidden % 32 == 0); }
bool layered_hidden_ok(int D, int hidden, int num_layers, bool anyh) {
    return D > 0 && layered_width_ok(hidden, anyh) && num_layers >= 1 && num_layers <= kLayeredMaxLayers;
}
// what a refusal says of the width
const char* layered_width_rule(bool anyh) { return anyh ? "1..1024" : "a multiple of 32, 32..1024"; }
size_t layered_act_plane_bytes(int N, int hidden) { return ((size_t)N * hidden * sizeof(float) + 63) & ~(size_t)63; }

// the layered layout's 4 (L + 1) + 1 offsets, each with what lies at it inside the bucket
int layered_offsets_check(const int* offsets, int D, int A, int continuous, int hidden, int L, int n_params, const char* who) {
    const int per = 2 * (L + 1), n_off = 2 * per + 1;
    for (int i = 0; i < n_off; ++i) {
        const int net = i / per, j = i % per, l = j / 2;
        const int out = i == 2 * per ? 0 : (l < L ? hidden : (net ? 1 : A));
        long long need;
        if (i == 2 * per) need = continuous ? A : 0;
        else if (j & 1) need = out;
        else need = (long long)out * (l == 0 ? D : hidden);
        AURPPO_REQUIRE(offsets[i] >= 0 && (long long)offsets[i] + need <= (long long)n_params, AURPPO_EINVAL,
                       "%s: layout offset %d (%d) outside the bucket of %d", who, i, offsets[i], n_params);
    }
    return AURPPO_OK;
}

// The layered update step's one workspace: per net and hidden layer an (M, hidden) activation array (the gradient with respect to the
// layer's pre-activation takes its place on the way down), the operand copy of the product in flight, the weight-gradient slices
// (with the bias builds' partial column sums), K13's workspace, and clip + Adam's for the minibatch call.
struct LayeredStepWs {
    float* act;              // [net][layer] planes of `plane` bytes
    size_t plane;
    void *wop, *wgrad, *head, *clip;
    size_t bytes;
};
LayeredStepWs layered_step_carve(void* workspace, int M, int D, int A, int width, int L) {
    const int hidden = layered_padded(width);          // every plane and product of the step is the padded shape's
    aurppo_mlp::WsCarver c(workspace);
    LayeredStepWs w;
    w.plane = layered_act_plane_bytes(M, hidden);
    w.act = c.take<float>((size_t)2 * L * w.plane, 64);
    w.wop = c.take<char>(aurppo_conv3x3_wop_bytes(D > hidden ? D : hidden, hidden), 64);
    const size_t wg0 = aurppo_linear_wgrad_bias_ws_bytes(M, hidden, D), wg = aurppo_linear_wgrad_bias_ws_bytes(M, hidden, hidden);
    w.wgrad = c.take<char>(wg0 > wg ? wg0 : wg, 64);
    w.head = c.take<char>(aurppo_head_ppo_wa_workspace_bytes(M, hidden, A), 64);     // the old entry's figure at A <= 16
    w.clip = c.take<char>(aurppo_clip_workspace_bytes(0), 64);
    w.bytes = c.bytes;
    return w;
}

// ---- the layered update step: mlp_ppo_step's contract on the same products.  Per net: layer 0 through the index (k_linear, bias + tanh
// in the epilogue), layers 1 .. L - 1; K13 (statistics, the kernel, its fold); then per net from the last layer down the weight gradient
// (k_linear_wgrad + fold) and the input gradient with tanh' (k_linear).  The weight gradient of a layer below the last runs the BIAS
// build, which leaves the layer's bias gradient (K13 writes the last layers').  Per product two launches (operand copy + k_linear,
// or k_linear_wgrad + fold): 2 (2 L) + 3 + 2 (2 L + 2 (L - 1)) = 12 L - 1 launches, no allocation, no host synchronisation.
int layered_step_impl(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A, int continuous,
                      int hidden, int num_layers, const float* params, const int* offsets, int n_params, float* grads, double clip,
                      double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace, void* stream,
                      bool anyh, int max_a, const char* who) {
    AURPPO_REQUIRE(obs && rec && idx && params && offsets && grads && out_scalars && workspace, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(M > 0 && D > 0 && num_layers >= 1 && num_layers <= kLayeredMaxLayers, AURPPO_ESHAPE, "%s: M=%d, D=%d, %d layers (1..%d)",
                   who, M, D, num_layers, kLayeredMaxLayers);
    const int Hp = layered_padded(hidden);             // the planes' and products' width; `hidden` stays the bucket's
    AURPPO_REQUIRE(layered_width_ok(hidden, anyh) && head_shape_ok_upto(Hp, A, continuous, max_a), AURPPO_ESHAPE,
                   "%s: hidden=%d (%s), A=%d (1..%d, Categorical: 2..%d)", who, hidden, layered_width_rule(anyh), A, max_a, max_a);
    AURPPO_REQUIRE(actions || (continuous ? A : 1) <= 12, AURPPO_ESHAPE, "%s: packed records hold at most 12 action floats (A=%d)", who, A);
    AURPPO_REQUIRE(vloss_mode >= 0 && vloss_mode <= 2, AURPPO_EINVAL, "%s: vloss_mode %d", who, vloss_mode);
    AURPPO_REQUIRE(aligned_to(obs, 16) && aligned_to(rec, 16) && aligned_to(workspace, 64), AURPPO_EINVAL,
                   "%s: obs / rec not 16-byte / workspace not 64-byte aligned", who);
    const int L = num_layers, per = 2 * (L + 1);
    if (const int rc = layered_offsets_check(offsets, D, A, continuous, hidden, L, n_params, who)) return rc;
    const LayeredStepWs w = layered_step_carve(workspace, M, D, A, hidden, L);
    auto h = [&](int net, int l) { return reinterpret_cast<float*>(reinterpret_cast<char*>(w.act) + (size_t)(net * L + l) * w.plane); };
    for (int net = 0; net < 2; ++net) {
        const int* o = offsets + net * per;
        if (const int rc = linear_product(obs, params + o[0], params + o[1], 1, h(net, 0), M, D, hidden, 0, D, Hp, w.wop, stream, idx, nullptr))
            return rc;
        for (int l = 1; l < L; ++l)
            if (const int rc = linear_product(h(net, l - 1), params + o[2 * l], params + o[2 * l + 1], 1, h(net, l), M, hidden, hidden, 0, Hp, Hp,
                                              w.wop, stream, nullptr, nullptr))
                return rc;
    }
    const int lay[7] = {offsets[2 * L], offsets[2 * L + 1], offsets[per + 2 * L], offsets[per + 2 * L + 1], offsets[2 * per],
                        offsets[2 * L - 1], offsets[per + 2 * L - 1]};
    if (const int rc = head_ppo_run("aurppo_head_ppo_f32", h(0, L - 1), h(1, L - 1), h(0, L - 1), h(1, L - 1), actions, rec, idx, M, Hp, hidden,
                                    A, continuous, params, lay, n_params, grads, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars,
                                    w.head, stream, max_a))
        return rc;
    for (int net = 0; net < 2; ++net) {
        const int* o = offsets + net * per;          // h(net, L - 1) now holds gz of the last layer; the lower layers follow in place
        for (int l = L - 1; l > 0; --l) {
            if (const int rc = linear_wgrad_product(h(net, l), h(net, l - 1), nullptr, grads + o[2 * l], l == L - 1 ? nullptr : grads + o[2 * l + 1],
                                                    M, Hp, Hp, hidden, hidden, w.wgrad, stream))
                return rc;
            if (const int rc = linear_product(h(net, l), params + o[2 * l], nullptr, 2, h(net, l - 1), M, hidden, hidden, 1, Hp, Hp, w.wop, stream,
                                              nullptr, h(net, l - 1)))
                return rc;
        }
        if (const int rc = linear_wgrad_product(h(net, 0), obs, idx, grads + o[0], L == 1 ? nullptr : grads + o[1], M, Hp, D, hidden, D, w.wgrad,
                                                stream))
            return rc;
    }
    return AURPPO_OK;
}

size_t layered_wop_bytes(int D, int hidden, int num_layers, bool anyh) {
    if (!layered_hidden_ok(D, hidden, num_layers, anyh)) return 0;
    const int Hp = layered_padded(hidden);
    return 2 * (aurppo_linear_wop_bytes(D, Hp) + (size_t)(num_layers - 1) * aurppo_linear_wop_bytes(Hp, Hp));
}

// The parameters stand still for the T steps of a rollout, so the operand-order copies of the 2 L hidden-layer matrices are built once,
// into a caller-owned buffer: [net][layer], each copy aurppo_linear_wop_bytes(its K, hidden) bytes.
// (at a width that is no multiple of 32 each copy is the padded product's, aurppo_linear_wop_bytes(its K, Hp), from k_linear_prep_pad)
int layered_prep_impl(const float* params, const int* offsets, int n_params, int D, int hidden, int num_layers, void* wop, void* stream,
                      bool anyh, const char* who) {
    AURPPO_REQUIRE(params && offsets && wop, AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(layered_hidden_ok(D, hidden, num_layers, anyh), AURPPO_ESHAPE, "%s: D=%d (1 or more), hidden=%d (%s), %d layers (1..%d)", who,
                   D, hidden, layered_width_rule(anyh), num_layers, kLayeredMaxLayers);
    AURPPO_REQUIRE(aligned_to(wop, 16), AURPPO_EINVAL, "%s: operand buffer not 16-byte aligned", who);
    const int per = 2 * (num_layers + 1), Hp = layered_padded(hidden);
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < num_layers; ++l) {
            const int o = offsets[net * per + 2 * l];
            AURPPO_REQUIRE(o >= 0 && (long long)o + (long long)hidden * (l ? hidden : D) <= (long long)n_params, AURPPO_EINVAL,
                           "%s: layout offset %d (%d) outside the bucket of %d", who, net * per + 2 * l, o, n_params);
        }
    char* at = reinterpret_cast<char*>(wop);
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < num_layers; ++l) {
            const int K = l ? hidden : D, Kg = l ? Hp : D;
            const float* const w = params + offsets[net * per + 2 * l];
            if (const int rc = Hp == hidden ? linear_prep(w, K, hidden, 0, reinterpret_cast<unsigned short*>(at), (hipStream_t)stream)
                                            : linear_prep_pad(w, K, hidden, 0, Kg, Hp, reinterpret_cast<unsigned short*>(at), (hipStream_t)stream))
                return rc;
            at += aurppo_linear_wop_bytes(Kg, Hp);
        }
    return AURPPO_OK;
}

}  // namespace

extern "C" size_t aurppo_mlp_layered_wop_bytes(int D, int hidden, int num_layers) { return layered_wop_bytes(D, hidden, num_layers, false); }
extern "C" size_t aurppo_mlp_layered_anyh_wop_bytes(int D, int hidden, int num_layers) { return layered_wop_bytes(D, hidden, num_layers, true); }
extern "C" int aurppo_mlp_layered_prep_f32(const float* params, const int* offsets, int n_params, int D, int hidden, int num_layers,
                                           void* wop, void* stream) {
    return layered_prep_impl(params, offsets, n_params, D, hidden, num_layers, wop, stream, false, "aurppo_mlp_layered_prep_f32");
}
extern "C" int aurppo_mlp_layered_anyh_prep_f32(const float* params, const int* offsets, int n_params, int D, int hidden, int num_layers,
                                                void* wop, void* stream) {
    return layered_prep_impl(params, offsets, n_params, D, hidden, num_layers, wop, stream, true, "aurppo_mlp_layered_anyh_prep_f32");
}

// ---- the layered rollout step: per net, the hidden layers on k_linear (bias + tanh in the epilogue) from the prepared operand
// copies (aurppo_mlp_layered_prep_f32), then K14.  2 L + 1 launches; the value alone: the critic only, L + 1.
extern "C" size_t aurppo_mlp_layered_act_workspace_bytes(int N, int hidden) {
    if (N <= 0 || hidden <= 0) return 0;
    return 4 * layered_act_plane_bytes(N, hidden);      // two activation planes per net, written in turn
}
// ... at any hidden width 1 .. 1024: the planes are (N, Hp)
extern "C" size_t aurppo_mlp_layered_anyh_act_workspace_bytes(int N, int hidden) {
    if (N <= 0 || !layered_width_ok(hidden, true)) return 0;
    return 4 * layered_act_plane_bytes(N, layered_padded(hidden));
}

namespace {

// The rollout step behind both entries.  paired: per layer ONE launch of the paired small-tile product for both nets (k_linear_pair),
// L + 1 launches with K14; without noise the critic alone on the single small-tile product (k_linear_small), L + 1 as well.  The
// bits are the unpaired route's: a row's result does not depend on the tile (linear_body.h).
int layered_act_impl(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden, int num_layers,
                     const float* params, const int* offsets, int n_params, float* actions, float* logp, float* value, const void* wop,
                     void* workspace, void* stream, bool paired, bool anyh, int max_a, const char* who) {
    AURPPO_REQUIRE(obs && params && offsets && value && wop && workspace && (!noise || (actions && logp)), AURPPO_EINVAL, "%s: null pointer",
                   who);
    AURPPO_REQUIRE(N > 0 && D > 0 && num_layers >= 1 && num_layers <= kLayeredMaxLayers, AURPPO_ESHAPE, "%s: N=%d, D=%d, %d layers (1..%d)",
                   who, N, D, num_layers, kLayeredMaxLayers);
    const int Hp = layered_padded(hidden);             // the planes' and products' width; `hidden` stays the bucket's
    AURPPO_REQUIRE(layered_width_ok(hidden, anyh) && head_shape_ok_upto(Hp, A, continuous, max_a), AURPPO_ESHAPE,
                   "%s: hidden=%d (%s), A=%d (1..%d, Categorical: 2..%d)", who, hidden, layered_width_rule(anyh), A, max_a, max_a);
    AURPPO_REQUIRE(aligned_to(obs, 16) && aligned_to(wop, 16) && aligned_to(workspace, 64), AURPPO_EINVAL,
                   "%s: obs / operand copies not 16-byte / workspace not 64-byte aligned", who);
    AURPPO_REQUIRE((!noise || (aligned_to(noise, 4) && aligned_to(actions, 4) && aligned_to(logp, 4))) && aligned_to(value, 4),
                   AURPPO_EINVAL, "%s: noise / outputs not 4-byte aligned", who);
    const int L = num_layers, per = 2 * (L + 1);
    if (const int rc = layered_offsets_check(offsets, D, A, continuous, hidden, L, n_params, who)) return rc;
    const size_t plane = layered_act_plane_bytes(N, Hp);
    const char* const wbase = reinterpret_cast<const char*>(wop);
    const size_t net_wop = aurppo_linear_wop_bytes(D, Hp) + (size_t)(L - 1) * aurppo_linear_wop_bytes(Hp, Hp);
    auto out = [&](int net, int l) { return reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + (size_t)(2 * net + (l & 1)) * plane); };
    const int first = noise ? 0 : 1;                   // the live nets are [first, 2): both, or the critic alone
    const bool pair = paired && first == 0;
    LinOps ops[2] = {};                                // (a net that does not run keeps its null pointers: K14 is not handed an actor)
    size_t at = 0;                                     // layer l's operand copy inside its net's
    for (int l = 0; l < L; ++l) {
        const int K = l ? Hp : D;
        for (int net = first; net < 2; ++net)
            ops[net] = {l ? out(net, l - 1) : obs, wbase + net * net_wop + at, params + offsets[net * per + 2 * l + 1], out(net, l)};
        for (int net = first; net < (pair ? 1 : 2); ++net)          // one launch for both nets, or one per live net on the chosen tile
            if (const int rc = aurppo_linear_forward(who, paired, pair ? 2 : 1, ops + net, 1, N, K, Hp, stream, hidden)) return rc;
        at += aurppo_linear_wop_bytes(K, Hp);
    }
    const int lay[5] = {offsets[2 * L], offsets[2 * L + 1], offsets[per + 2 * L], offsets[per + 2 * L + 1], offsets[2 * per]};
    return head_act_launch(ops[0].y, ops[1].y, noise, N, Hp, hidden, A, continuous, params, lay, actions, logp, value, (hipStream_t)stream);
}

}  // namespace

// The entries.  The aurppo_mlp_layered_anyh_* ones take their siblings' argument lists and any hidden width 1 .. 1024; at a multiple of 32
// both run the same calls.  The aurppo_mlp_layered_wa_* ones take the anyh entries' argument lists and widths and up to 32 actions; at
// A <= 16 they run the anyh entries' calls.
#define AURPPO_LAYERED_ACT_ENTRY(NAME, PAIRED, ANYH, MAX_A)                                                                                \
    extern "C" int NAME(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden, int num_layers,             \
                        const float* params, const int* offsets, int n_params, float* actions, float* logp, float* value, const void* wop, \
                        void* workspace, void* stream) {                                                                                   \
        return layered_act_impl(obs, noise, N, D, A, continuous, hidden, num_layers, params, offsets, n_params, actions, logp, value, wop, \
                                workspace, stream, PAIRED, ANYH, MAX_A, #NAME);                                                            \
    }
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_act_f32, false, false, 16)
// The same step on the small-M products, both nets' layer l in one launch: same arguments, same buffers, same bits, L + 1 launches.
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_act_paired_f32, true, false, 16)
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_anyh_act_f32, false, true, 16)
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_anyh_act_paired_f32, true, true, 16)
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_wa_act_f32, false, true, 32)
AURPPO_LAYERED_ACT_ENTRY(aurppo_mlp_layered_wa_act_paired_f32, true, true, 32)
#undef AURPPO_LAYERED_ACT_ENTRY

namespace {

size_t layered_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers, bool anyh, int max_a) {
    if (M <= 0 || D <= 0 || num_layers < 1 || num_layers > kLayeredMaxLayers || !layered_width_ok(hidden, anyh) ||
        !head_shape_ok_upto(layered_padded(hidden), A, 1, max_a))
        return 0;
    return layered_step_carve(nullptr, M, D, A, hidden, num_layers).bytes;
}

// The step, then clip + Adam (aurppo_clip_adam_f32's two launches) over [0, n_params) on the same stream.
int layered_minibatch_impl(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A, int continuous,
                           int hidden, int num_layers, float* params, const int* offsets, int n_params, float* grads, double clip,
                           double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, float* exp_avg, float* exp_avg_sq,
                           double max_norm, const float* lr_dev, float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                           void* workspace, void* stream, bool anyh, int max_a, const char* who) {
    AURPPO_REQUIRE(exp_avg && exp_avg_sq && lr_dev && step_dev && out_norm, AURPPO_EINVAL, "%s: null optimizer pointer", who);
    if (const int rc = layered_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, num_layers, params, offsets, n_params, grads,
                                         clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, anyh, max_a, who))
        return rc;
    const LayeredStepWs w = layered_step_carve(workspace, M, D, A, hidden, num_layers);
    return aurppo_clip_adam_f32(params, grads, exp_avg, exp_avg_sq, n_params, n_params, max_norm, lr_dev, step_dev, beta1, beta2, eps, out_norm,
                                w.clip, stream);
}

}  // namespace

extern "C" size_t aurppo_mlp_layered_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers) {
    return layered_step_workspace_bytes(M, D, A, hidden, num_layers, false, 16);
}
extern "C" size_t aurppo_mlp_layered_anyh_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers) {
    return layered_step_workspace_bytes(M, D, A, hidden, num_layers, true, 16);
}
extern "C" size_t aurppo_mlp_layered_wa_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers) {
    return layered_step_workspace_bytes(M, D, A, hidden, num_layers, true, 32);
}

#define AURPPO_LAYERED_STEP_ENTRY(NAME, ANYH, MAX_A)                                                                                       \
    extern "C" int NAME(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A, int continuous, \
                        int hidden, int num_layers, const float* params, const int* offsets, int n_params, float* grads, double clip,      \
                        double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace, void* stream) { \
        return layered_step_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, num_layers, params, offsets, n_params, grads, clip,  \
                                 ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, ANYH, MAX_A, #NAME);             \
    }
AURPPO_LAYERED_STEP_ENTRY(aurppo_mlp_layered_step_f32, false, 16)
AURPPO_LAYERED_STEP_ENTRY(aurppo_mlp_layered_anyh_step_f32, true, 16)
AURPPO_LAYERED_STEP_ENTRY(aurppo_mlp_layered_wa_step_f32, true, 32)
#undef AURPPO_LAYERED_STEP_ENTRY

#define AURPPO_LAYERED_MINIBATCH_ENTRY(NAME, ANYH, MAX_A)                                                                                  \
    extern "C" int NAME(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A, int continuous, \
                        int hidden, int num_layers, float* params, const int* offsets, int n_params, float* grads, double clip,            \
                        double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, float* exp_avg,                 \
                        float* exp_avg_sq, double max_norm, const float* lr_dev, float* step_dev, double beta1, double beta2, double eps,  \
                        float* out_norm, void* workspace, void* stream) {                                                                  \
        return layered_minibatch_impl(obs, actions, rec, idx, M, D, A, continuous, hidden, num_layers, params, offsets, n_params, grads,   \
                                      clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, exp_avg, exp_avg_sq, max_norm, lr_dev,   \
                                      step_dev, beta1, beta2, eps, out_norm, workspace, stream, ANYH, MAX_A, #NAME);                       \
    }
AURPPO_LAYERED_MINIBATCH_ENTRY(aurppo_mlp_layered_minibatch_f32, false, 16)
AURPPO_LAYERED_MINIBATCH_ENTRY(aurppo_mlp_layered_anyh_minibatch_f32, true, 16)
AURPPO_LAYERED_MINIBATCH_ENTRY(aurppo_mlp_layered_wa_minibatch_f32, true, 32)
#undef AURPPO_LAYERED_MINIBATCH_ENTRY
