// vi_host_occupancy.h -- the host path of the forward pass of a policy (vi_occupancy.h).
// It reads the handle's cells and options only: V, pi, kenv and the protocol state stay as they are.
// Part of the single translation unit vi.hip: included after vi_host_eval.h (launch_on_eval_shape).
#pragma once

namespace {

constexpr int kOccMaxN = 1 << 20;  // the error word's row field (kFhMaxH)

// n_steps -> N: the horizon on a finite-horizon handle (0 or the horizon itself), the caller's on horizon 0
int occupancy_supported(const mgdp_vi *vi, int32_t T, int32_t n_steps, int *N_out) {
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    MGDP_CHECK(vi->d.model == MGDP_MODEL_XYD, MGDP_E_UNSUPPORTED,
               "occupancy is defined for the XYD model: the DoorKey DP has no slip, so its forward pass from one "
               "start state is the env's rollout (mgdp_envs_rollout with a trace, rollout(trace=True))");
    MGDP_CHECK(vi->HW <= 1024, MGDP_E_UNSUPPORTED, "occupancy needs W*H <= 1024");
    MGDP_CHECK(vi->d.B <= kFhMaxB, MGDP_E_UNSUPPORTED, "occupancy: batch %d exceeds the policy error word", vi->d.B);
    const int H = vi->d.horizon;
    int N = n_steps;
    if (H > 0) {
        MGDP_CHECK(n_steps == 0 || n_steps == H, MGDP_E_INVALID,
                   "occupancy: n_steps = %d on a finite-horizon handle: 0 or the horizon %d", n_steps, H);
        MGDP_CHECK(H <= kOccMaxN, MGDP_E_UNSUPPORTED, "occupancy: horizon %d exceeds the policy error word", H);
        N = H;
    } else {
        MGDP_CHECK(n_steps >= 1 && n_steps <= kOccMaxN, MGDP_E_INVALID, "occupancy: n_steps = %d is outside [1, %d]",
                   n_steps, kOccMaxN);
    }
    MGDP_CHECK(T == 1 || T == N, MGDP_E_INVALID, "policy rows T = %d: 1 (stationary) or the %d steps", T, N);
    *N_out = N;
    return 0;
}

// disc[0] = 1, disc[t+1] = fl(g * disc[t]); wg[t] = fl(disc[t] * rgoal[t]) on a finite horizon, else disc[t];
// wl[t] = fl(disc[t] * dc) -- built in T on the host, as tests/occupancy_ref.py builds them
template <typename T>
int occupancy_tables(mgdp_vi *vi, int N) {
    if (vi->d_occ_tab && vi->occ_tab_n == N) return 0;
    (void)hipFree(vi->d_occ_tab);
    vi->d_occ_tab = nullptr;
    vi->occ_tab_n = 0;
    std::vector<T> tab((size_t)3 * N);
    const T g = (T)vi->d.gamma, dc = (T)vi->d.death_cost;
    const int H = vi->d.horizon;
    T d = (T)1;
    for (int t = 0; t < N; ++t) {
        tab[t] = d;
        const T rg = H > 0 ? (T)(1.0 - 0.9 * ((double)(t + 1) / (double)H)) : (T)1;  // _reward(t+1, H), as d_rgoal holds it
        tab[(size_t)N + t] = H > 0 ? d * rg : d;
        tab[(size_t)2 * N + t] = d * dc;
        d = g * d;
    }
    MGDP_HIP(hipMalloc(&vi->d_occ_tab, tab.size() * sizeof(T)));
    MGDP_HIP(hipMemcpyAsync(vi->d_occ_tab, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    vi->occ_tab_n = N;
    return 0;
}

template <typename T, bool SLIP, bool ND>
struct OccupancyF {  // + (time-indexed policy, mu_t stored)
    static int run(mgdp_vi *vi, const int8_t *d_pi, bool ti, const int32_t *d_start, const void *d_mu0, int N,
                   void *d_mu, void *d_occ, void *d_ret, void *d_mu_t) {
        return fan_out2(ti, d_mu_t != nullptr, [&](auto TI, auto MT) {
            if (int rc = launch_on_eval_shape(vi, vi_occupancy_kernel<T, SLIP, ND, decltype(TI)::value, decltype(MT)::value>,
                                              make_coef<T>(vi), vi->d_cells, d_pi, d_start, (const T *)d_mu0,
                                              (const T *)vi->d_occ_tab, (T *)d_mu, (T *)d_occ, (T *)d_ret, (T *)d_mu_t,
                                              vi->d_occ_err, N))
                return rc;
            MGDP_HIP(hipGetLastError());
            return 0;
        });
    }
};
template <typename T, typename... Args>
int dispatch_occupancy_t(mgdp_vi *vi, Args... args) {
    return fan_out2(vi->d.slip_p >= 0.0, vi->d.lava_mode == MGDP_LAVA_NODEATH, [&](auto SLIP, auto ND) {
        return OccupancyF<T, decltype(SLIP)::value, decltype(ND)::value>::run(vi, args...);
    });
}

// One launch of exactly N steps on device pointers, then the two error words (drains the stream).
int occupancy_run(mgdp_vi *vi, const int8_t *d_pi, int T, const int32_t *d_start, const void *d_mu0, int N, void *d_mu,
                  void *d_occ, void *d_ret, void *d_mu_t) {
    if (!vi->d_occ_err) MGDP_HIP(hipMalloc((void **)&vi->d_occ_err, 2 * sizeof(unsigned long long)));
    if (int rc = vi->tsize == 4 ? occupancy_tables<float>(vi, N) : occupancy_tables<double>(vi, N)) return rc;
    MGDP_HIP(hipMemsetAsync(vi->d_occ_err, 0xff, 2 * sizeof(unsigned long long), vi->stream));
    const bool ti = T != 1;
    if (int rc = vi->tsize == 4 ? dispatch_occupancy_t<float>(vi, d_pi, ti, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t)
                                : dispatch_occupancy_t<double>(vi, d_pi, ti, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t))
        return rc;
    unsigned long long err[2] = {kEvalNoError, kEvalNoError};
    MGDP_HIP(hipMemcpyAsync(err, vi->d_occ_err, sizeof(err), hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    if (err[1] != kEvalNoError) {
        const int grid = (int)(err[1] >> 32), state = (int)(uint32_t)(err[1] & 0xffffffffull);
        MGDP_CHECK(d_mu0, MGDP_E_INVALID, "start: grid %d state %d is outside [0, %d) or absorbing (wall, goal, lava)", grid,
                   state, vi->S);
        MGDP_CHECK(false, MGDP_E_INVALID, "mu0: grid %d state %d is absorbing (wall, goal, lava) and holds mass", grid, state);
    }
    MGDP_CHECK(err[0] == kEvalNoError, MGDP_E_INVALID, "policy: grid %d t %d state %d: action %d is outside [0, %d)",
               (int)(err[0] >> kFhGridShift), (int)((err[0] >> kFhRowShift) & (unsigned long long)(kFhMaxH - 1)),
               (int)((err[0] >> 8) & 0x3fffu), (int)(int8_t)(err[0] & 0xffu), vi->A);
    return 0;
}

int occupancy_args(const void *pi, const void *start, const void *mu0, const void *mu) {
    MGDP_CHECK(pi && mu, MGDP_E_INVALID, "null argument");
    MGDP_CHECK((start != nullptr) != (mu0 != nullptr), MGDP_E_INVALID, "exactly one of start and mu0 must be given");
    return 0;
}

int occupancy_device(mgdp_vi *vi, const int8_t *d_pi, int32_t T, const int32_t *d_start, const void *d_mu0,
                     int32_t n_steps, void *d_mu, void *d_occ, void *d_ret, void *d_mu_t) {
    int N = 0;
    if (int rc = occupancy_args(d_pi, d_start, d_mu0, d_mu)) return rc;
    if (int rc = occupancy_supported(vi, T, n_steps, &N)) return rc;
    MGDP_CHECK((((uintptr_t)d_pi | (uintptr_t)d_mu0 | (uintptr_t)d_mu | (uintptr_t)d_occ | (uintptr_t)d_ret | (uintptr_t)d_mu_t) & 15u) == 0 &&
                   ((uintptr_t)d_start & 3u) == 0,
               MGDP_E_INVALID, "occupancy: the device pointers must be 16-byte aligned (start: 4-byte)");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    return occupancy_run(vi, d_pi, T, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t);
}

int occupancy_host(mgdp_vi *vi, const int8_t *pi, int32_t T, const int32_t *start, const void *mu0, int32_t n_steps,
                   void *mu, void *occ, void *ret, void *mu_t) {
    int N = 0;
    if (int rc = occupancy_args(pi, start, mu0, mu)) return rc;
    if (int rc = occupancy_supported(vi, T, n_steps, &N)) return rc;
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const size_t BS = (size_t)vi->d.B * vi->S, plane = BS * vi->tsize;
    // staging: [0] the policy rows, [1] start / mu0, [2] the three planes, [3] mu_t
    const size_t need[4] = {(size_t)T * BS, start ? sizeof(int32_t) * vi->d.B : plane, 3 * plane, mu_t ? (size_t)N * plane : 0};
    for (int i = 0; i < 4; ++i) {
        if (need[i] <= vi->occ_stage_cap[i]) continue;
        (void)hipFree(vi->d_occ_stage[i]);
        vi->d_occ_stage[i] = nullptr;
        vi->occ_stage_cap[i] = 0;
        MGDP_HIP(hipMalloc(&vi->d_occ_stage[i], need[i]));
        vi->occ_stage_cap[i] = need[i];
    }
    unsigned char *out = (unsigned char *)vi->d_occ_stage[2];
    MGDP_HIP(hipMemcpyAsync(vi->d_occ_stage[0], pi, need[0], hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipMemcpyAsync(vi->d_occ_stage[1], start ? (const void *)start : mu0, need[1], hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));  // the caller's buffers are free when this returns
    if (int rc = occupancy_run(vi, (const int8_t *)vi->d_occ_stage[0], T, start ? (const int32_t *)vi->d_occ_stage[1] : nullptr,
                               start ? nullptr : vi->d_occ_stage[1], N, out, occ ? out + plane : nullptr,
                               ret ? out + 2 * plane : nullptr, mu_t ? vi->d_occ_stage[3] : nullptr))
        return rc;
    MGDP_HIP(hipMemcpyAsync(mu, out, plane, hipMemcpyDeviceToHost, vi->stream));
    if (occ) MGDP_HIP(hipMemcpyAsync(occ, out + plane, plane, hipMemcpyDeviceToHost, vi->stream));
    if (ret) MGDP_HIP(hipMemcpyAsync(ret, out + 2 * plane, plane, hipMemcpyDeviceToHost, vi->stream));
    if (mu_t) MGDP_HIP(hipMemcpyAsync(mu_t, vi->d_occ_stage[3], (size_t)N * plane, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

}  // namespace
