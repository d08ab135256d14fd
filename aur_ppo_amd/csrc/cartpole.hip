// CartPole-v1 on the device, and the whole rollout of the default MLP policy on it as one launch.
//   * k_cartpole_reset          -- episode 0 of every env: the state from its reset draw, the fp32 observation.
//   * k_cartpole_step (K15)     -- one env step, one thread per env: aur_ppo_amd/envs.py CartPoleVecEnv.step's formulas in fp64 in the
//                                  same association (gym's classic_control cart-pole: Euler, tau 0.02), termination, truncation,
//                                  auto-reset and the finished episode's length.
//   * k_cartpole_rollout (K16)  -- the T steps of src/ppo.py:201-205 for K8's shape (2 x 64, Categorical, A = 2, D = 4): one workgroup
//                                  per 32-env tile stages both nets' weights and its envs ONCE and loops over the steps -- the two
//                                  state / terminal row stores, K8's three layers and sampler, K15's step on the 32 lanes that
//                                  sampled, the four row stores behind it.  The LDS plan, the weight staging and the three layers
//                                  are mlp_act.h's (ActLds, act_stage_weights, act_forward): K8's passages as functions (k_mlp_act
//                                  takes the plan and keeps the other two inline: the note above it, mlp.hip); the sampler is
//                                  ppo_math.h's, shared with K8.  Tiles share nothing: no inter-workgroup traffic, only
//                                  __syncthreads() between phases.  An MFMA row depends on its own operand row alone, so every value
//                                  is, bit for bit, what T x (K8, K15) leave.
// The state is fp64 (as gym and the host class keep it; observations are its fp32 rounding).  A reset is a function of (seed, global
// env index, episode number) alone -- Philox4x32-10 on the counter (env0 + n, episode, 0, 0) under the key (seed lo, seed hi) -- so it
// does not depend on how a rollout is cut into launches.  The dynamics and the draw are one __device__ function each, shared by
// K15 and K16.
#include "mlp_act.h"
#include "philox.h"

using namespace aurppo_mlp;

namespace {

constexpr int kD = 4;    // CartPole's observation: x, x_dot, theta, theta_dot
constexpr int kA = 2;    // push left / push right

struct CartConst {
    double gravity, masscart, masspole, length, force_mag, tau, theta_lim, x_lim;
    int max_steps;
    int env0;            // global index of env 0 (a rank's first env)
    uint32_t k0, k1;     // the seed's low and high words
};

struct CartEnv {
    double s[4];
    int steps, episode;
};

// The reset state of global env `genv`, episode `episode`: component j = -0.05 + 0.1 * u_j, u_j the top 24 bits of word j in [0, 1)
__device__ __forceinline__ void cart_reset_draw(double s[4], int genv, int episode, const CartConst& c) {
    uint32_t x[4];
    philox4x32_10((uint32_t)genv, (uint32_t)episode, 0u, 0u, c.k0, c.k1, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = -0.05 + 0.1 * ((double)(x[j] >> 8) * 0x1p-24);
}

// One step of env `genv`: CartPoleVecEnv.step, operation for operation.  Leaves the next state (the reset draw of the next episode where
// this one ended), returns done; ep_len: the finished episode's length, or 0.
__device__ __forceinline__ bool cart_step(CartEnv& e, float action, int genv, const CartConst& c, int& ep_len) {
    const double x = e.s[0], xd = e.s[1], th = e.s[2], thd = e.s[3];
    const double force = action == 1.0f ? c.force_mag : -c.force_mag;
    const double ct = cos(th), st = sin(th);
    const double total_mass = c.masscart + c.masspole;
    const double pml = c.masspole * c.length;
    const double temp = (force + pml * thd * thd * st) / total_mass;
    const double thacc = (c.gravity * st - ct * temp) / (c.length * (4.0 / 3.0 - c.masspole * ct * ct / total_mass));
    const double xacc = temp - pml * thacc * ct / total_mass;
    e.s[0] = x + c.tau * xd;
    e.s[1] = xd + c.tau * xacc;
    e.s[2] = th + c.tau * thd;
    e.s[3] = thd + c.tau * thacc;
    e.steps += 1;
    const bool term = fabs(e.s[0]) > c.x_lim || fabs(e.s[2]) > c.theta_lim;
    const bool done = term || e.steps >= c.max_steps;
    ep_len = done ? e.steps : 0;
    if (done) {
        e.episode += 1;
        cart_reset_draw(e.s, genv, e.episode, c);
        e.steps = 0;
    }
    return done;
}

__device__ __forceinline__ CartEnv cart_load(const double* state, const int32_t* steps, const int32_t* episode, int n) {
    CartEnv e;
#pragma unroll
    for (int j = 0; j < 4; ++j) e.s[j] = state[(size_t)n * 4 + j];
    e.steps = steps[n];
    e.episode = episode[n];
    return e;
}
__device__ __forceinline__ void cart_store(const CartEnv& e, double* state, int32_t* steps, int32_t* episode, int n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) state[(size_t)n * 4 + j] = e.s[j];
    steps[n] = e.steps;
    episode[n] = e.episode;
}

__global__ __launch_bounds__(256) void k_cartpole_reset(double* __restrict__ state, int32_t* __restrict__ steps, int32_t* __restrict__ episode,
                                                        float* __restrict__ obs, int N, const CartConst c) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    CartEnv e;
    e.steps = 0;
    e.episode = 0;
    cart_reset_draw(e.s, c.env0 + n, 0, c);
    cart_store(e, state, steps, episode, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) obs[(size_t)n * 4 + j] = (float)e.s[j];
}

__global__ __launch_bounds__(256) void k_cartpole_step(double* __restrict__ state, int32_t* __restrict__ steps, int32_t* __restrict__ episode,
                                                       const float* __restrict__ action, float* __restrict__ obs, float* __restrict__ reward,
                                                       float* __restrict__ done, int32_t* __restrict__ ep_len, int N, const CartConst c) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    CartEnv e = cart_load(state, steps, episode, n);
    int len;
    const bool d = cart_step(e, action[n], c.env0 + n, c, len);
    cart_store(e, state, steps, episode, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) obs[(size_t)n * 4 + j] = (float)e.s[j];
    reward[n] = 1.0f;
    done[n] = d ? 1.0f : 0.0f;
    ep_len[n] = len;
}

struct RolloutArgs {
    double* state;          // (N, 4)
    int32_t* steps;         // (N,)
    int32_t* episode;       // (N,)
    float* obs_io;          // (N, 4): in, the current observation; out, the one after T steps
    float* done_io;         // (N,):   in, the current done flag; out, the last step's
    const float* noise;     // (T, N) uniform [0, 1)
    const float* params;
    float* states;          // (T, N, 4)
    float* terminals;       // (T, N)
    float* actions;         // (T, N)
    float* logp;            // (T, N)
    float* values;          // (T, N)
    float* rewards;         // (T, N)
    int32_t* ep_len;        // (T, N)
    int N, T;
    MlpLayout L;
    CartConst c;
};

// K8's LDS plan without the Gaussian head's log-std rows, its weight staging and its three layers: mlp_act.h (ActLds,
// act_stage_weights, act_forward).  Here: the zero fill of sX and the step's row writes from registers, the Categorical sampler's call,
// the env lanes.
__global__ __launch_bounds__(256, 1) void k_cartpole_rollout(const RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ActLds s(lds);
    float* const sX = s.sX;
    const float* const sOut = s.sOut;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * R;
    // ---- once per launch: the weights (as k_mlp_act stages them), a zero sX, this lane's env
#pragma unroll
    for (int u = 0; u < R * H / kThreads; ++u) {
        const int e = tid + u * kThreads;
        sX[(e >> 6) * LD + (e & 63)] = 0.0f;     // columns kD .. stay zero for the whole launch, and so do a ragged tile's dead rows
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) act_stage_weights(s, a.params, a.L, kD, kA, n);
    // the 32 lanes that sample own one env each for the T steps: its state, observation and done flag live in their registers
    const int n = row0 + tid;
    const bool live = tid < R && n < a.N;
    CartEnv env = {};
    float ob[kD] = {0.0f, 0.0f, 0.0f, 0.0f}, dn = 0.0f;
    if (live) {
        env = cart_load(a.state, a.steps, a.episode, n);
#pragma unroll
        for (int j = 0; j < kD; ++j) ob[j] = a.obs_io[(size_t)n * kD + j];
        dn = a.done_io[n];
    }
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        const size_t tn = (size_t)t * a.N + n;
        float u = 0.0f;
        if (live) {
            u = a.noise[tn];            // asked for here, used behind the three layers
#pragma unroll
            for (int j = 0; j < kD; ++j) {
                a.states[tn * kD + j] = ob[j];
                sX[tid * LD + j] = ob[j];
            }
            a.terminals[tn] = dn;
        }
        __syncthreads();
        act_forward(s);
        // (the next step's sX / sOut writes are behind its own barriers: nothing here races with them)
        if (live) {
            const float* mu = sOut + tid * LDO;
            a.values[tn] = sOut[(R + tid) * LDO];
            const float lse = cat_lse(mu, kA);
            float lp;
            const float act = (float)cat_sample(mu, kA, lse, u, lp);
            a.actions[tn] = act;
            a.logp[tn] = lp;
            int len;
            const bool d = cart_step(env, act, a.c.env0 + n, a.c, len);
#pragma unroll
            for (int j = 0; j < kD; ++j) ob[j] = (float)env.s[j];
            dn = d ? 1.0f : 0.0f;
            a.rewards[tn] = 1.0f;
            a.ep_len[tn] = len;
        }
    }
    if (live) {
        cart_store(env, a.state, a.steps, a.episode, n);
#pragma unroll
        for (int j = 0; j < kD; ++j) a.obs_io[(size_t)n * kD + j] = ob[j];
        a.done_io[n] = dn;
    }
}

int fill_const(CartConst& c, const char* who, int N, int env0, uint32_t seed_lo, uint32_t seed_hi, double gravity, double masscart,
               double masspole, double length, double force_mag, double tau, double theta_lim, double x_lim, int max_steps) {
    AURPPO_REQUIRE(N > 0 && env0 >= 0 && (long long)env0 + N <= 0x7fffffffLL, AURPPO_ESHAPE, "%s: N=%d env0=%d", who, N, env0);
    AURPPO_REQUIRE(max_steps > 0 && masscart + masspole > 0.0 && length > 0.0, AURPPO_EINVAL, "%s: max_steps=%d masscart=%g masspole=%g length=%g",
                   who, max_steps, masscart, masspole, length);
    c.gravity = gravity; c.masscart = masscart; c.masspole = masspole; c.length = length; c.force_mag = force_mag; c.tau = tau;
    c.theta_lim = theta_lim; c.x_lim = x_lim; c.max_steps = max_steps; c.env0 = env0; c.k0 = seed_lo; c.k1 = seed_hi;
    return AURPPO_OK;
}

}  // namespace

extern "C" int aurppo_cartpole_reset(double* state, int32_t* steps, int32_t* episode, float* obs, int N, int env0, uint32_t seed_lo,
                                     uint32_t seed_hi, void* stream) {
    AURPPO_REQUIRE(state && steps && episode && obs, AURPPO_EINVAL, "aurppo_cartpole_reset: null pointer");
    CartConst c = {};
    // (a reset reads the key and env0 alone; the checks on the dynamics' constants are given values that pass)
    if (const int rc = fill_const(c, "aurppo_cartpole_reset", N, env0, seed_lo, seed_hi, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1)) return rc;
    hipLaunchKernelGGL(k_cartpole_reset, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, steps, episode, obs, N, c);
    AURPPO_LAUNCH_CHECK("k_cartpole_reset");
    return AURPPO_OK;
}

extern "C" int aurppo_cartpole_step(double* state, int32_t* steps, int32_t* episode, const float* action, float* obs, float* reward,
                                    float* done, int32_t* ep_len, int N, int env0, uint32_t seed_lo, uint32_t seed_hi, double gravity,
                                    double masscart, double masspole, double length, double force_mag, double tau, double theta_lim,
                                    double x_lim, int max_steps, void* stream) {
    AURPPO_REQUIRE(state && steps && episode && action && obs && reward && done && ep_len, AURPPO_EINVAL,
                   "aurppo_cartpole_step: null pointer");
    CartConst c = {};
    if (const int rc = fill_const(c, "aurppo_cartpole_step", N, env0, seed_lo, seed_hi, gravity, masscart, masspole, length, force_mag, tau,
                                  theta_lim, x_lim, max_steps))
        return rc;
    hipLaunchKernelGGL(k_cartpole_step, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, steps, episode, action, obs, reward,
                       done, ep_len, N, c);
    AURPPO_LAUNCH_CHECK("k_cartpole_step");
    return AURPPO_OK;
}

extern "C" int aurppo_cartpole_rollout_f32(double* state, int32_t* steps, int32_t* episode, float* obs_io, float* done_io, const float* noise,
                                           int N, int T, int D, int A, int continuous, int hidden, int num_layers, const float* params,
                                           const int* layout_h, int n_params, float* states, float* terminals, float* actions, float* logp,
                                           float* values, float* rewards, int32_t* ep_len, int env0, uint32_t seed_lo, uint32_t seed_hi,
                                           double gravity, double masscart, double masspole, double length, double force_mag, double tau,
                                           double theta_lim, double x_lim, int max_steps, void* stream) {
    const char* who = "aurppo_cartpole_rollout_f32";
    AURPPO_REQUIRE(state && steps && episode && obs_io && done_io && noise && params && layout_h && states && terminals && actions && logp &&
                       values && rewards && ep_len,
                   AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(N > 0 && T > 0 && n_params > 0, AURPPO_ESHAPE, "%s: N=%d T=%d n_params=%d", who, N, T, n_params);
    AURPPO_REQUIRE(hidden == H && num_layers == 2, AURPPO_ESHAPE, "%s: %d layers of hidden_dim=%d (only 2 x %d is built)", who, num_layers,
                   hidden, H);
    AURPPO_REQUIRE(D == kD && A == kA && !continuous, AURPPO_ESHAPE,
                   "%s: state_dim=%d action_dim=%d continuous=%d (CartPole: %d floats, a Categorical head of %d)", who, D, A, continuous, kD, kA);
    RolloutArgs a;
    if (const int rc = fill_layout(a.L, layout_h, 0, n_params, who)) return rc;     // a Categorical head reads no log-std
    if (const int rc = fill_const(a.c, who, N, env0, seed_lo, seed_hi, gravity, masscart, masspole, length, force_mag, tau, theta_lim, x_lim,
                                  max_steps))
        return rc;
    a.state = state; a.steps = steps; a.episode = episode; a.obs_io = obs_io; a.done_io = done_io; a.noise = noise; a.params = params;
    a.states = states; a.terminals = terminals; a.actions = actions; a.logp = logp; a.values = values; a.rewards = rewards; a.ep_len = ep_len;
    a.N = N; a.T = T;
    return launch_dyn_lds<k_cartpole_rollout>("k_cartpole_rollout", (N + R - 1) / R, kThreads, ActLds::bytes(false), ActLds::bytes(false),
                                              (hipStream_t)stream, a);
}
