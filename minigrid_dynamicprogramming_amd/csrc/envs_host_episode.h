// envs_host_episode.h -- episodes on resident envs: tabular policies (policy lookup and the fused rollout,
// DESIGN.md section 16), the slip and explore stream tables (sections 17 and 18) and tabular Q-learning
// (section 18).  Per entry point: the checks, the kernel chosen, the launch, and the host forms' staging in
// the roll scratch.  Part of envs.hip (see envs_host.h).
#pragma once

namespace {

// ---- tabular policies on resident envs (envs_rollout.h) --------------------
constexpr int kRollLdsMax = 160 * 1024 - 2048;  // the 64 padded planes; the rest is the staging pass's words

int model_states(const mgdp_envs *E, int32_t model) { return E->W * E->H * (model == MGDP_MODEL_XYD ? 4 : 16); }

int roll_check(const mgdp_envs *E, int32_t model, const void *pi, int32_t T, int *S) {
    MGDP_CHECK(E && pi, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(model == MGDP_MODEL_XYD || model == MGDP_MODEL_DOORKEY, MGDP_E_INVALID, "unknown model %d", model);
    MGDP_CHECK(T >= 1, MGDP_E_INVALID, "T must be >= 1 (1 = a stationary policy), got %d", T);
    MGDP_CHECK(!E->d_cont, MGDP_E_UNSUPPORTED, "Box contents planes are in use on this handle: outside both models");
    *S = model_states(E, model);
    return 0;
}

// The episode kernels' cell reader: LDS planes wherever a wave's 64 fit, unless MGDP_ROLLOUT_READER says hbm.
bool roll_on_lds(const mgdp_envs *E) {
    const bool fits = kRollWave * roll_stride(E->HWp) <= kRollLdsMax;
    return E->roll_reader < 0 ? fits : (E->roll_reader == 1 && fits);
}

// A trace: states [len][B] and actions [len][B], or none (null, null, 0).
struct TraceBufs {
    int32_t *state;
    int8_t *act;
    int len;
};

// Device buffers: both or neither.
int trace_device(int32_t *state, int8_t *act, int32_t len, TraceBufs *t) {
    const bool trace = state && act;
    MGDP_CHECK(trace || (!state && !act), MGDP_E_INVALID, "a trace needs both of its buffers");
    *t = trace ? TraceBufs{state, act, len} : TraceBufs{nullptr, nullptr, 0};
    return 0;
}

// Host buffers: both and len > 0, or else none is used.
int trace_host(int32_t *state, int8_t *act, int32_t len, TraceBufs *t) {
    const bool trace = state && act && len > 0;
    MGDP_CHECK(trace || (!state && !act) || len == 0, MGDP_E_INVALID, "a trace needs both of its buffers");
    *t = trace ? TraceBufs{state, act, len} : TraceBufs{nullptr, nullptr, 0};
    return 0;
}

// One wave per 64 envs (envs_rollout_kernel, envs_qlearn_kernel): smem bytes of dynamic LDS, the trace
// cleared to -1 (entries no step fills stay so), the launch timed like every other.  args follow the
// env's own buffers in the kernel's signature.
template <typename K, typename... Args>
int launch_episode(mgdp_envs *E, K k, int smem, const TraceBufs &t, const Args &...args) {
    if (smem > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    if (t.len > 0) {
        MGDP_HIP(hipMemsetAsync(t.state, 0xff, sizeof(int32_t) * (size_t)t.len * E->B, E->stream));
        MGDP_HIP(hipMemsetAsync(t.act, 0xff, (size_t)t.len * E->B, E->stream));
    }
    return launch_timed(E, k, dim3((E->B + kRollWave - 1) / kRollWave), dim3(kRollWave), smem, env_geo(E), E->d_cell, E->d_agent,
                        E->d_carry, E->d_max, args...);
}

int launch_policy_actions(mgdp_envs *E, int32_t model, const int8_t *d_pi, int32_t T, int S, int32_t *d_actions,
                          int32_t *d_status) {
    auto k = model == MGDP_MODEL_XYD ? envs_policy_actions_kernel<kRollXYD> : envs_policy_actions_kernel<kRollDoorKey>;
    return launch_timed(E, k, dim3((E->B + 255) / 256), dim3(256), 0, env_geo(E), E->d_cell, E->d_agent, E->d_carry, d_pi, T, S,
                        d_actions, d_status);
}

SlipArgs slip_args(const mgdp_envs *E) { return SlipArgs{E->slip_p, E->slip_ra, E->slip.state, E->slip.half}; }
SlipArgs explore_args(const mgdp_envs *E) { return SlipArgs{1.0, -1, E->explore.state, E->explore.half}; }

using RolloutKernel = void (*)(EnvGeo, uint8_t *, int32_t *, int32_t *, const int32_t *, RolloutArgs, SlipArgs);
template <bool SLIP>
RolloutKernel rollout_kernel(int32_t model, bool lds) {
    return model == MGDP_MODEL_XYD ? (lds ? envs_rollout_kernel<kRollXYD, true, SLIP> : envs_rollout_kernel<kRollXYD, false, SLIP>)
                                   : (lds ? envs_rollout_kernel<kRollDoorKey, true, SLIP>
                                          : envs_rollout_kernel<kRollDoorKey, false, SLIP>);
}

int launch_rollout(mgdp_envs *E, int32_t model, const RolloutArgs &r) {
    const bool lds = roll_on_lds(E);
    const RolloutKernel k = E->slip.on ? rollout_kernel<true>(model, lds) : rollout_kernel<false>(model, lds);
    return launch_episode(E, k, lds ? kRollWave * roll_stride(E->HWp) : 0, TraceBufs{r.tr_state, r.tr_act, r.trace_len}, r,
                          slip_args(E));
}

int launch_slip_actions(mgdp_envs *E, const int32_t *d_in, int32_t *d_out) {
    return launch_timed(E, envs_slip_actions_kernel, dim3((E->B + 255) / 256), dim3(256), 0, E->B, slip_args(E), d_in, d_out);
}

// ---- stream tables: slip and explore (DESIGN.md sections 17 and 18) -------------------------------
// Stream b of the table becomes default_rng(seed0 + b); mask [B] (host) keeps the streams of its zero
// entries.  entry names the caller in the refusal of a masked first seeding.
int seed_streams(mgdp_envs *E, StreamTable &t, uint64_t seed0, const uint8_t *mask, const char *entry) {
    MGDP_CHECK(t.on || !mask, MGDP_E_INVALID, "the first %s seeds every stream: no mask", entry);
    DeviceGuard guard(E->device);
    const size_t B = E->B;
    if (!t.state) MGDP_HIP(hipMalloc((void **)&t.state, sizeof(uint64_t) * 4 * B));
    if (!t.half) MGDP_HIP(hipMalloc((void **)&t.half, sizeof(uint32_t) * 2 * B));
    if (mask) {
        if (!E->d_stream_mask) MGDP_HIP(hipMalloc((void **)&E->d_stream_mask, B));
        MGDP_HIP(hipMemcpyAsync(E->d_stream_mask, mask, B, hipMemcpyHostToDevice, E->stream));
    }
    hipLaunchKernelGGL(envs_slip_seed_kernel, dim3((E->B + 255) / 256), dim3(256), 0, E->stream, E->B, seed0,
                       mask ? E->d_stream_mask : nullptr, SlipArgs{1.0, -1, t.state, t.half});
    MGDP_HIP(hipGetLastError());
    if (mask) MGDP_HIP(hipStreamSynchronize(E->stream));  // the caller's mask may go once this returns
    t.on = true;
    return 0;
}

int read_streams(mgdp_envs *E, const StreamTable &t, uint64_t *state, uint32_t *half) {
    DeviceGuard guard(E->device);
    const size_t B = E->B;
    if (download(E, state, t.state, sizeof(uint64_t) * 4 * B) || download(E, half, t.half, sizeof(uint32_t) * 2 * B))
        return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

// ---- tabular Q-learning on resident envs (envs_qlearn.h) --------------------
int q_model_check(const mgdp_envs *E, int32_t model, int32_t n_act, int *S, int *A) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(model == MGDP_MODEL_XYD || model == MGDP_MODEL_DOORKEY, MGDP_E_INVALID, "unknown model %d", model);
    *A = model == MGDP_MODEL_XYD ? 7 : 5;
    *S = model_states(E, model);
    MGDP_CHECK(n_act >= 1 && n_act <= *A, MGDP_E_INVALID, "n_act must be in 1..%d, got %d", *A, n_act);
    return 0;
}

int q_learn_check(const mgdp_envs *E, int32_t model, int32_t n_steps, double alpha, double gamma, double eps, int32_t n_act,
                  int32_t unit_goal, int32_t trace_len, int *S, int *A) {
    if (int rc = q_model_check(E, model, n_act, S, A)) return rc;
    MGDP_CHECK(n_steps > 0, MGDP_E_INVALID, "n_steps must be > 0, got %d", n_steps);
    MGDP_CHECK(eps >= 0.0 && eps <= 1.0, MGDP_E_INVALID, "eps must be in [0, 1], got %g", eps);  // NaN fails both
    MGDP_CHECK(alpha == alpha && gamma == gamma, MGDP_E_INVALID, "alpha and gamma must not be NaN");
    MGDP_CHECK(unit_goal == 0 || unit_goal == 1, MGDP_E_INVALID, "unit_goal must be 0 or 1, got %d", unit_goal);
    MGDP_CHECK(trace_len >= 0, MGDP_E_INVALID, "trace_len must be >= 0, got %d", trace_len);
    MGDP_CHECK(E->explore.on, MGDP_E_INVALID, "no explore streams on this handle (mgdp_envs_set_explore)");
    MGDP_CHECK(!E->d_cont, MGDP_E_UNSUPPORTED, "Box contents planes are in use on this handle: outside both models");
    MGDP_CHECK(model == MGDP_MODEL_XYD || kRollWave * roll_stride(E->HWp) <= kRollLdsMax, MGDP_E_UNSUPPORTED,
               "DoorKey Q-learning restores mutated planes from HBM into LDS: 64 planes of %d x %d do not fit", E->W, E->H);
    return 0;
}

using QLearnKernel = void (*)(EnvGeo, const uint8_t *, const int32_t *, const int32_t *, const int32_t *, QLearnArgs, SlipArgs,
                              SlipArgs);
template <bool SLIP>
QLearnKernel qlearn_kernel(int32_t model, bool lds) {
    return model == MGDP_MODEL_DOORKEY ? envs_qlearn_kernel<kRollDoorKey, true, SLIP>
           : lds                       ? envs_qlearn_kernel<kRollXYD, true, SLIP>
                                       : envs_qlearn_kernel<kRollXYD, false, SLIP>;
}

int launch_qlearn(mgdp_envs *E, int32_t model, const QLearnArgs &q) {
    // MGDP_ROLLOUT_READER chooses the XYD reader as for the rollout; DoorKey always steps on LDS (q_learn_check)
    const bool lds = model == MGDP_MODEL_DOORKEY || roll_on_lds(E);
    const QLearnKernel k = E->slip.on ? qlearn_kernel<true>(model, lds) : qlearn_kernel<false>(model, lds);
    return launch_episode(E, k, lds ? kRollWave * roll_stride(E->HWp) : 0, TraceBufs{q.tr_state, q.tr_act, q.trace_len}, q,
                          explore_args(E), slip_args(E));
}

int launch_q_greedy(mgdp_envs *E, int32_t model, int S, const double *d_Q, int32_t n_act, int8_t *d_pi, double *d_Vq) {
    const long long n = (long long)E->B * S;
    auto k = model == MGDP_MODEL_XYD ? envs_q_greedy_kernel<7> : envs_q_greedy_kernel<5>;
    return launch_timed(E, k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, n, d_Q, n_act, d_pi, d_Vq);
}

// ---- the host forms: inputs staged in the roll scratch, the launch, the outputs the caller asked for ----
int policy_actions_host(mgdp_envs *E, int32_t model, const int8_t *pi, int32_t T, int S, int32_t *actions, int32_t *status) {
    const size_t B = E->B, n_pi = (size_t)T * B * S;
    RollCursor c;
    const size_t o_pi = c.take(n_pi);
    if (int rc = grow(E, E->roll, c.end)) return rc;
    int8_t *d_pi = roll_at<int8_t>(E, o_pi);
    MGDP_HIP(hipMemcpyAsync(d_pi, pi, n_pi, hipMemcpyHostToDevice, E->stream));
    if (int rc = launch_policy_actions(E, model, d_pi, T, S, E->d_act, E->d_status)) return rc;
    if (download(E, actions, E->d_act, 4 * B) || download(E, status, E->d_status, 4 * B)) return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

int rollout_host(mgdp_envs *E, int32_t model, const int8_t *pi, int32_t T, int S, int32_t n_max, int32_t *steps, double *ret,
                 uint8_t *terminated, uint8_t *truncated, int32_t *status, const TraceBufs &h) {
    const size_t B = E->B, n_pi = (size_t)T * B * S, n_tr = (size_t)h.len * B;
    RollCursor c;
    const size_t o_pi = c.take(n_pi), o_ts = c.take(4 * n_tr), o_ta = c.take(n_tr);
    if (int rc = grow(E, E->roll, c.end)) return rc;
    int8_t *d_pi = roll_at<int8_t>(E, o_pi);
    const TraceBufs d{roll_at<int32_t>(E, o_ts), roll_at<int8_t>(E, o_ta), h.len};
    MGDP_HIP(hipMemcpyAsync(d_pi, pi, n_pi, hipMemcpyHostToDevice, E->stream));
    // the step entry points' per-env buffers serve as outputs: d_act holds the step counts
    const RolloutArgs r{d_pi, T, S, n_max, d.len, E->d_act, E->d_rew, E->d_term, E->d_trunc, E->d_status, d.state, d.act};
    if (int rc = launch_rollout(E, model, r)) return rc;
    if (download(E, steps, E->d_act, 4 * B) || download(E, ret, E->d_rew, 8 * B) || download(E, terminated, E->d_term, B) ||
        download(E, truncated, E->d_trunc, B) || download(E, status, E->d_status, 4 * B) ||
        download(E, h.state, d.state, 4 * n_tr) || download(E, h.act, d.act, n_tr))
        return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

// q: the caller's parameters, its pointers unset.  Scratch: Q | episodes | wins | trace states | trace
// actions; steps, ret and status use the step buffers.
int q_learn_host(mgdp_envs *E, int32_t model, QLearnArgs q, int A, double *Q, int32_t *steps, int32_t *episodes, int32_t *wins,
                 double *ret, int32_t *status, const TraceBufs &h) {
    const size_t B = E->B, n_q = sizeof(double) * B * q.S * A, n_tr = (size_t)h.len * B;
    RollCursor c;
    const size_t o_q = c.take(n_q), o_ep = c.take(4 * B), o_wn = c.take(4 * B), o_ts = c.take(4 * n_tr), o_ta = c.take(n_tr);
    if (int rc = grow(E, E->roll, c.end)) return rc;
    double *d_Q = roll_at<double>(E, o_q);
    int32_t *d_ep = roll_at<int32_t>(E, o_ep), *d_wn = roll_at<int32_t>(E, o_wn);
    const TraceBufs d{roll_at<int32_t>(E, o_ts), roll_at<int8_t>(E, o_ta), h.len};
    MGDP_HIP(hipMemcpyAsync(d_Q, Q, n_q, hipMemcpyHostToDevice, E->stream));
    q.Q = d_Q; q.steps = E->d_act; q.episodes = d_ep; q.wins = d_wn; q.ret = E->d_rew; q.status = E->d_status;
    q.trace_len = d.len; q.tr_state = d.state; q.tr_act = d.act;
    if (int rc = launch_qlearn(E, model, q)) return rc;
    if (download(E, Q, d_Q, n_q) || download(E, steps, E->d_act, 4 * B) || download(E, episodes, d_ep, 4 * B) ||
        download(E, wins, d_wn, 4 * B) || download(E, ret, E->d_rew, 8 * B) || download(E, status, E->d_status, 4 * B) ||
        download(E, h.state, d.state, 4 * n_tr) || download(E, h.act, d.act, n_tr))
        return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

int q_greedy_host(mgdp_envs *E, int32_t model, int S, int A, const double *Q, int32_t n_act, int8_t *pi, double *Vq) {
    const size_t n = (size_t)E->B * S, n_q = sizeof(double) * n * A, n_v = sizeof(double) * n;
    RollCursor c;
    const size_t o_q = c.take(n_q), o_v = c.take(n_v), o_pi = c.take(n);
    if (int rc = grow(E, E->roll, c.end)) return rc;
    double *d_Q = roll_at<double>(E, o_q), *d_V = roll_at<double>(E, o_v);
    int8_t *d_pi = roll_at<int8_t>(E, o_pi);
    MGDP_HIP(hipMemcpyAsync(d_Q, Q, n_q, hipMemcpyHostToDevice, E->stream));
    if (int rc = launch_q_greedy(E, model, S, d_Q, n_act, d_pi, Vq ? d_V : nullptr)) return rc;
    if (download(E, pi, d_pi, n) || download(E, Vq, d_V, n_v)) return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

}  // namespace
