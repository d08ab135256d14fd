// Pendulum-v1 on the device behind the reference's continuous wrapper chain, and the whole rollout of the default Gaussian MLP policy
// on it as one launch.
//   * k_pendulum_reset          -- every env starts over: episode 0 from its reset draw, fresh statistics, the first normalised observation.
//   * k_pendulum_step (K17)     -- one env step, one thread per env: aur_ppo_amd/envs.py PendulumVecEnv.step's formulas in fp64 in the
//                                  same association (gym 0.26.2's classic_control pendulum, v1; ClipAction, NormalizeObservation, clip +-10,
//                                  NormalizeReward, clip +-10 per env), truncation at max_steps, auto-reset, the finished episode's
//                                  length and raw return.
//   * k_pendulum_rollout (K18)  -- the T steps of src/ppo.py:201-205 for K8's Gaussian shape (2 x 64, D = 3, A = 1): K16's design
//                                  (cartpole.hip) for the other head.  One workgroup per 32-env tile stages both nets' weights, the
//                                  log-std rows and its envs ONCE and loops over the steps -- the two state / terminal row stores,
//                                  mlp_act.h's three layers, ppo_math.h's Gaussian sampler, K17's step on the lane that owns the
//                                  env, the row stores behind it.  Tiles share nothing: no inter-workgroup traffic, only
//                                  __syncthreads() between phases.  Every value is, bit for bit, what T x (K8, K17) leave.
// Per-env state: one row of kS = 16 doubles (the Slot enum below; include/aurppo.h documents it) plus int32 steps / episode.  A reset
// is a function of (seed, global env index, episode number) alone -- Philox4x32-10 on the counter (env0 + n, episode, 1, 0) under the
// key (seed lo, seed hi); the third word keeps the stream apart from CartPole's.  The core step, one RunningMeanStd update and the
// reset draw are one __device__ function each, shared by K17 and K18.
#include "mlp_act.h"
#include "philox.h"

using namespace aurppo_mlp;

namespace {

constexpr int kD = 3;    // Pendulum's observation: cos th, sin th, thdot
constexpr int kA = 1;    // the torque
constexpr int kS = 16;   // doubles per env in the state block

enum Slot { sTh, sThd, sObsMean, sObsVar = sObsMean + kD, sObsCount = sObsVar + kD, sRetMean, sRetVar, sRetCount, sRet, sEpRet, sSpare };
static_assert(sSpare == 14 && sSpare <= kS, "the state block's layout (include/aurppo.h) has changed");

constexpr double kPi = 3.141592653589793;     // numpy's pi
constexpr double kNormGamma = 0.99;           // NormalizeReward's own discount (not the trainer's)
constexpr double kNormEps = 1e-8;             // both Normalize wrappers' epsilon
constexpr double kNormClip = 10.0;            // the TransformObservation / TransformReward clip
constexpr double kCount0 = 1e-4;              // RunningMeanStd's initial count

struct PendConst {
    double g, m, l, dt, max_speed, max_torque;
    int max_steps;
    int env0;            // global index of env 0 (a rank's first env)
    uint32_t k0, k1;     // the seed's low and high words
};

struct PendEnv {
    double th, thd;
    double om[kD], ov[kD], oc;    // NormalizeObservation's mean, var, count
    double rm, rv, rc;            // NormalizeReward's mean, var, count
    double ret;                   // its discounted return
    double epr;                   // RecordEpisodeStatistics' raw return
    int steps, episode;
};

__device__ __forceinline__ double clipd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }   // np.clip: NaN passes

// ((x + pi) % (2 pi)) - pi with numpy's floored %: fmod, then + 2 pi where the remainder is non-zero and negative
__device__ __forceinline__ double angle_normalize(double x) {
    double r = fmod(x + kPi, 2.0 * kPi);
    if (r != 0.0 && r < 0.0) r += 2.0 * kPi;
    return r - kPi;
}

// The reset state of global env `genv`, episode `episode`: th = -pi + 2 pi u_0, thdot = -1 + 2 u_1, u_j the top 24 bits of word j in [0, 1)
__device__ __forceinline__ void pend_reset_draw(double& th, double& thd, int genv, int episode, const PendConst& c) {
    uint32_t x[4];
    philox4x32_10((uint32_t)genv, (uint32_t)episode, 1u, 0u, c.k0, c.k1, x);
    th = -kPi + 2.0 * kPi * ((double)(x[0] >> 8) * 0x1p-24);
    thd = -1.0 + 2.0 * ((double)(x[1] >> 8) * 0x1p-24);
}

// The core step, PendulumVecEnv.step operation for operation: leaves (th', thdot'), returns the raw reward -cost
__device__ __forceinline__ double pend_core_step(double& th, double& thd, float action, const PendConst& c) {
    const double u = clipd((double)action, -c.max_torque, c.max_torque);
    const double an = angle_normalize(th);
    const double cost = an * an + 0.1 * (thd * thd) + 0.001 * (u * u);
    const double nthd = clipd(thd + (3.0 * c.g / (2.0 * c.l) * sin(th) + 3.0 / (c.m * (c.l * c.l)) * u) * c.dt, -c.max_speed, c.max_speed);
    th = th + nthd * c.dt;
    thd = nthd;
    return -cost;
}

// One RunningMeanStd.update with a batch of one (batch_var = 0, batch_count = 1) on one component; the caller bumps the count behind
// the components that share it
__device__ __forceinline__ void rms_update(double& mean, double& var, double count, double x) {
    const double delta = x - mean;
    const double tot = count + 1.0;
    mean = mean + delta / tot;
    const double M2 = var * count + delta * delta * count / tot;
    var = M2 / tot;
}

// The raw fp32 observation of the state as it stands, taken into the observation statistics
__device__ __forceinline__ void pend_take_obs(PendEnv& e, float raw[kD]) {
    raw[0] = (float)cos(e.th);
    raw[1] = (float)sin(e.th);
    raw[2] = (float)e.thd;
#pragma unroll
    for (int j = 0; j < kD; ++j) rms_update(e.om[j], e.ov[j], e.oc, (double)raw[j]);
    e.oc = e.oc + 1.0;
}
__device__ __forceinline__ void pend_norm_obs(const PendEnv& e, const float raw[kD], float ob[kD]) {
#pragma unroll
    for (int j = 0; j < kD; ++j) ob[j] = (float)clipd(((double)raw[j] - e.om[j]) / sqrt(e.ov[j] + kNormEps), -kNormClip, kNormClip);
}

__device__ __forceinline__ void pend_start(PendEnv& e, int genv, const PendConst& c, float ob[kD]) {
    e.steps = 0;
    e.episode = 0;
#pragma unroll
    for (int j = 0; j < kD; ++j) { e.om[j] = 0.0; e.ov[j] = 1.0; }
    e.oc = kCount0;
    e.rm = 0.0; e.rv = 1.0; e.rc = kCount0;
    e.ret = 0.0;
    e.epr = 0.0;
    pend_reset_draw(e.th, e.thd, genv, 0, c);
    float raw[kD];
    pend_take_obs(e, raw);
    pend_norm_obs(e, raw, ob);
}

// One step of env `genv` through the whole wrapper chain.  Leaves the next state (the reset draw of the next episode where this one
// was truncated), the normalised observation and reward; returns done; ep_len / ep_ret: the finished episode's length and raw
// return, or 0.
__device__ __forceinline__ bool pend_step(PendEnv& e, float action, int genv, const PendConst& c, float ob[kD], float& reward, int& ep_len,
                                          float& ep_ret) {
    const double r = pend_core_step(e.th, e.thd, action, c);
    e.steps += 1;
    e.epr = e.epr + r;
    const bool done = e.steps >= c.max_steps;      // a truncation: Pendulum never terminates
    float raw[kD];
    pend_take_obs(e, raw);                         // the final observation where done
    ep_len = done ? e.steps : 0;
    ep_ret = done ? (float)e.epr : 0.0f;
    if (done) {
        e.episode += 1;
        pend_reset_draw(e.th, e.thd, genv, e.episode, c);
        e.steps = 0;
        e.epr = 0.0;
        pend_take_obs(e, raw);                     // ... and the reset one behind it: gym's auto-reset
    }
    pend_norm_obs(e, raw, ob);
    e.ret = e.ret * kNormGamma + r;                // not cleared at a truncation
    rms_update(e.rm, e.rv, e.rc, e.ret);
    e.rc = e.rc + 1.0;
    reward = (float)clipd(r / sqrt(e.rv + kNormEps), -kNormClip, kNormClip);
    return done;
}

__device__ __forceinline__ PendEnv pend_load(const double* state, const int32_t* steps, const int32_t* episode, int n) {
    const double* s = state + (size_t)n * kS;
    PendEnv e;
    e.th = s[sTh]; e.thd = s[sThd];
#pragma unroll
    for (int j = 0; j < kD; ++j) { e.om[j] = s[sObsMean + j]; e.ov[j] = s[sObsVar + j]; }
    e.oc = s[sObsCount];
    e.rm = s[sRetMean]; e.rv = s[sRetVar]; e.rc = s[sRetCount];
    e.ret = s[sRet];
    e.epr = s[sEpRet];
    e.steps = steps[n];
    e.episode = episode[n];
    return e;
}
__device__ __forceinline__ void pend_store(const PendEnv& e, double* state, int32_t* steps, int32_t* episode, int n) {
    double* s = state + (size_t)n * kS;
    s[sTh] = e.th; s[sThd] = e.thd;
#pragma unroll
    for (int j = 0; j < kD; ++j) { s[sObsMean + j] = e.om[j]; s[sObsVar + j] = e.ov[j]; }
    s[sObsCount] = e.oc;
    s[sRetMean] = e.rm; s[sRetVar] = e.rv; s[sRetCount] = e.rc;
    s[sRet] = e.ret;
    s[sEpRet] = e.epr;
    steps[n] = e.steps;
    episode[n] = e.episode;
}

__global__ __launch_bounds__(256) void k_pendulum_reset(double* __restrict__ state, int32_t* __restrict__ steps, int32_t* __restrict__ episode,
                                                        float* __restrict__ obs, int N, const PendConst c) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    PendEnv e;
    float ob[kD];
    pend_start(e, c.env0 + n, c, ob);
    pend_store(e, state, steps, episode, n);
    state[(size_t)n * kS + sSpare] = 0.0;
    state[(size_t)n * kS + sSpare + 1] = 0.0;
#pragma unroll
    for (int j = 0; j < kD; ++j) obs[(size_t)n * kD + j] = ob[j];
}

__global__ __launch_bounds__(256) void k_pendulum_step(double* __restrict__ state, int32_t* __restrict__ steps, int32_t* __restrict__ episode,
                                                       const float* __restrict__ action, float* __restrict__ obs, float* __restrict__ reward,
                                                       float* __restrict__ done, int32_t* __restrict__ ep_len, float* __restrict__ ep_ret, int N,
                                                       const PendConst c) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    PendEnv e = pend_load(state, steps, episode, n);
    float ob[kD], rew, ret;
    int len;
    const bool d = pend_step(e, action[n], c.env0 + n, c, ob, rew, len, ret);
    pend_store(e, state, steps, episode, n);
#pragma unroll
    for (int j = 0; j < kD; ++j) obs[(size_t)n * kD + j] = ob[j];
    reward[n] = rew;
    done[n] = d ? 1.0f : 0.0f;
    ep_len[n] = len;
    ep_ret[n] = ret;
}

struct RolloutArgs {
    double* state;          // (N, 16)
    int32_t* steps;         // (N,)
    int32_t* episode;       // (N,)
    float* obs_io;          // (N, 3): in, the current observation; out, the one after T steps
    float* done_io;         // (N,):   in, the current done flag; out, the last step's
    const float* noise;     // (T, N, 1) standard normal
    const float* params;
    float* states;          // (T, N, 3)
    float* terminals;       // (T, N)
    float* actions;         // (T, N, 1)
    float* logp;            // (T, N)
    float* values;          // (T, N)
    float* rewards;         // (T, N)
    int32_t* ep_len;        // (T, N)
    float* ep_ret;          // (T, N)
    int N, T;
    MlpLayout L;
    PendConst c;
};

// K8's whole LDS plan (the log-std rows included), its weight staging and its three layers: mlp_act.h.  Here: the zero fill of sX and
// the step's row writes from registers, the Gaussian sampler's call, the env lanes.
__global__ __launch_bounds__(256, 1) void k_pendulum_rollout(const RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ActLds s(lds);
    float* const sX = s.sX;
    const float* const sOut = s.sOut;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * R;
    // ---- once per launch: the weights and the log-std rows (as k_mlp_act stages them), a zero sX, this lane's env
#pragma unroll
    for (int u = 0; u < R * H / kThreads; ++u) {
        const int e = tid + u * kThreads;
        sX[(e >> 6) * LD + (e & 63)] = 0.0f;     // columns kD .. stay zero for the whole launch, and so do a ragged tile's dead rows
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) act_stage_weights(s, a.params, a.L, kD, kA, n);
    act_stage_logstd(s, a.params, a.L, kA, true);
    // the 32 lanes that sample own one env each for the T steps: its state, observation and done flag live in their registers
    const int n = row0 + tid;
    const bool live = tid < R && n < a.N;
    PendEnv env = {};
    float ob[kD] = {0.0f, 0.0f, 0.0f}, dn = 0.0f;
    if (live) {
        env = pend_load(a.state, a.steps, a.episode, n);
#pragma unroll
        for (int j = 0; j < kD; ++j) ob[j] = a.obs_io[(size_t)n * kD + j];
        dn = a.done_io[n];
    }
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        const size_t tn = (size_t)t * a.N + n;
        float eps = 0.0f;
        if (live) {
            eps = a.noise[tn];          // asked for here, used behind the three layers
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
            a.values[tn] = sOut[(R + tid) * LDO];
            // K8 folds a row's log-prob over eight lanes, dims lj and lj + 8 per lane: at A = 1 that is this one term added to a 0.0f
            // accumulator and seven lanes' 0.0f added behind it, which change no bit of it
            float act, lp = 0.0f;
            lp += gauss_sample(sOut[tid * LDO], s.sSd[0], s.sLs[0], eps, act);
            a.actions[tn] = act;
            a.logp[tn] = lp;
            float rew, ret;
            int len;
            const bool d = pend_step(env, act, a.c.env0 + n, a.c, ob, rew, len, ret);
            dn = d ? 1.0f : 0.0f;
            a.rewards[tn] = rew;
            a.ep_len[tn] = len;
            a.ep_ret[tn] = ret;
        }
    }
    if (live) {
        pend_store(env, a.state, a.steps, a.episode, n);
#pragma unroll
        for (int j = 0; j < kD; ++j) a.obs_io[(size_t)n * kD + j] = ob[j];
        a.done_io[n] = dn;
    }
}

int fill_const(PendConst& c, const char* who, int N, int env0, uint32_t seed_lo, uint32_t seed_hi, double g, double m, double l, double dt,
               double max_speed, double max_torque, int max_steps) {
    AURPPO_REQUIRE(N > 0 && env0 >= 0 && (long long)env0 + N <= 0x7fffffffLL, AURPPO_ESHAPE, "%s: N=%d env0=%d", who, N, env0);
    AURPPO_REQUIRE(max_steps > 0 && m > 0.0 && l > 0.0 && max_speed >= 0.0 && max_torque >= 0.0, AURPPO_EINVAL,
                   "%s: max_steps=%d m=%g l=%g max_speed=%g max_torque=%g", who, max_steps, m, l, max_speed, max_torque);
    c.g = g; c.m = m; c.l = l; c.dt = dt; c.max_speed = max_speed; c.max_torque = max_torque; c.max_steps = max_steps;
    c.env0 = env0; c.k0 = seed_lo; c.k1 = seed_hi;
    return AURPPO_OK;
}

}  // namespace

extern "C" int aurppo_pendulum_reset(double* state, int32_t* steps, int32_t* episode, float* obs, int N, int env0, uint32_t seed_lo,
                                     uint32_t seed_hi, void* stream) {
    AURPPO_REQUIRE(state && steps && episode && obs, AURPPO_EINVAL, "aurppo_pendulum_reset: null pointer");
    PendConst c = {};
    // (a reset reads the key and env0 alone; the checks on the dynamics' constants are given values that pass)
    if (const int rc = fill_const(c, "aurppo_pendulum_reset", N, env0, seed_lo, seed_hi, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1)) return rc;
    hipLaunchKernelGGL(k_pendulum_reset, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, steps, episode, obs, N, c);
    AURPPO_LAUNCH_CHECK("k_pendulum_reset");
    return AURPPO_OK;
}

extern "C" int aurppo_pendulum_step(double* state, int32_t* steps, int32_t* episode, const float* action, float* obs, float* reward,
                                    float* done, int32_t* ep_len, float* ep_ret, int N, int env0, uint32_t seed_lo, uint32_t seed_hi,
                                    double g, double m, double l, double dt, double max_speed, double max_torque, int max_steps,
                                    void* stream) {
    AURPPO_REQUIRE(state && steps && episode && action && obs && reward && done && ep_len && ep_ret, AURPPO_EINVAL,
                   "aurppo_pendulum_step: null pointer");
    PendConst c = {};
    if (const int rc = fill_const(c, "aurppo_pendulum_step", N, env0, seed_lo, seed_hi, g, m, l, dt, max_speed, max_torque, max_steps)) return rc;
    hipLaunchKernelGGL(k_pendulum_step, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, steps, episode, action, obs, reward,
                       done, ep_len, ep_ret, N, c);
    AURPPO_LAUNCH_CHECK("k_pendulum_step");
    return AURPPO_OK;
}

extern "C" int aurppo_pendulum_rollout_f32(double* state, int32_t* steps, int32_t* episode, float* obs_io, float* done_io, const float* noise,
                                           int N, int T, int D, int A, int continuous, int hidden, int num_layers, const float* params,
                                           const int* layout_h, int n_params, float* states, float* terminals, float* actions, float* logp,
                                           float* values, float* rewards, int32_t* ep_len, float* ep_ret, int env0, uint32_t seed_lo,
                                           uint32_t seed_hi, double g, double m, double l, double dt, double max_speed, double max_torque,
                                           int max_steps, void* stream) {
    const char* who = "aurppo_pendulum_rollout_f32";
    AURPPO_REQUIRE(state && steps && episode && obs_io && done_io && noise && params && layout_h && states && terminals && actions && logp &&
                       values && rewards && ep_len && ep_ret,
                   AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(N > 0 && T > 0 && n_params > 0, AURPPO_ESHAPE, "%s: N=%d T=%d n_params=%d", who, N, T, n_params);
    AURPPO_REQUIRE(hidden == H && num_layers == 2, AURPPO_ESHAPE, "%s: %d layers of hidden_dim=%d (only 2 x %d is built)", who, num_layers,
                   hidden, H);
    AURPPO_REQUIRE(D == kD && A == kA && continuous, AURPPO_ESHAPE,
                   "%s: state_dim=%d action_dim=%d continuous=%d (Pendulum: %d floats, a Gaussian head of %d)", who, D, A, continuous, kD, kA);
    RolloutArgs a;
    if (const int rc = fill_layout(a.L, layout_h, 1, n_params, who)) return rc;
    if (const int rc = fill_const(a.c, who, N, env0, seed_lo, seed_hi, g, m, l, dt, max_speed, max_torque, max_steps)) return rc;
    a.state = state; a.steps = steps; a.episode = episode; a.obs_io = obs_io; a.done_io = done_io; a.noise = noise; a.params = params;
    a.states = states; a.terminals = terminals; a.actions = actions; a.logp = logp; a.values = values; a.rewards = rewards; a.ep_len = ep_len;
    a.ep_ret = ep_ret; a.N = N; a.T = T;
    return launch_dyn_lds<k_pendulum_rollout>("k_pendulum_rollout", (N + R - 1) / R, kThreads, ActLds::bytes(true), ActLds::bytes(true),
                                              (hipStream_t)stream, a);
}
