// vi_host_eval.h -- the host path of policy evaluation, improvement and policy iteration (DESIGN.md sections 13
// and 19; kernels in vi_eval.h and vi_eval_opts.h).  One implementation per operation, over (pi, T rows, V_t):
// the plain ABI names are its strict form (no option handle, T = 1, no V_t), the *_opts names check T / V_t and
// take any handle.  An evaluation is the solve's protocol on vi_eval_kernel: every grid to its own stop, the
// grids that stopped with dV != 0 to K = max k_e, then the global rule sweep by sweep if dV(K) >= tol
// (vi_rule.h); on a finite horizon it is one launch of exactly H sweeps.  Also here: the timed launch of one
// workgroup per grid that vi_host_occupancy.h (on eval_shape) and vi_host_qvalues.h (on its own shape) share.
// Part of the single translation unit vi.hip: included after vi_host_order.h.
#pragma once

namespace {

inline bool option_handle(const mgdp_vi *vi) { return vi->d.horizon > 0 || vi->d.lava_mode != MGDP_LAVA_TERMINAL; }

// `opts`: the call came through an *_opts name.  The plain names refuse an option handle; the limits of the
// option kernels (one thread per cell, the finite-horizon error word) bind an option handle only -- a plain
// handle above 1024 cells takes vi_eval_kernel's strided form through either name.
int eval_supported(const mgdp_vi *vi, const char *what, bool opts) {
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED, MGDP_E_UNSUPPORTED, "%s runs on the fused method only", what);
    if (!opts) {
        MGDP_CHECK(vi->d.horizon == 0, MGDP_E_UNSUPPORTED, "%s is defined for the discounted problem (horizon 0)", what);
        MGDP_CHECK(vi->d.lava_mode == MGDP_LAVA_TERMINAL, MGDP_E_UNSUPPORTED,
                   "%s needs terminal lava (NoDeath makes V negative)", what);
    }
    const bool oh = option_handle(vi);
    MGDP_CHECK(!oh || vi->HW <= 1024, MGDP_E_UNSUPPORTED, "%s under horizon / lava options needs W*H <= 1024", what);
    const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
    MGDP_CHECK(s.lds <= 160 * 1024, MGDP_E_UNSUPPORTED,
               "%s: grid too large for the LDS-resident evaluation (%d B > 160 KiB)", what, s.lds);
    MGDP_CHECK(!oh || (vi->d.horizon <= kFhMaxH && vi->d.B <= kFhMaxB), MGDP_E_UNSUPPORTED,
               "%s: horizon %d / batch %d exceed the policy error word", what, vi->d.horizon, vi->d.B);
    return 0;
}
// improvement and policy iteration: an *_opts name refuses a finite horizon in its own words, first
int greedy_supported(const mgdp_vi *vi, const char *what, bool opts) {
    MGDP_CHECK(!opts || vi->d.horizon == 0, MGDP_E_UNSUPPORTED,
               "%s is refused on a finite horizon: its greedy step is the solve itself", what);
    return eval_supported(vi, what, opts);
}
// the policy rows T and V_t of an *_opts name (the plain names: T = 1, no V_t)
int eval_rows_supported(const mgdp_vi *vi, int32_t T, const void *V_t) {
    const int H = vi->d.horizon;
    MGDP_CHECK(T == 1 || (H > 0 && T == H), MGDP_E_INVALID,
               "policy rows T = %d: 1 (stationary)%s", T, H > 0 ? " or the handle's horizon" : " on a horizon-0 handle");
    MGDP_CHECK(!(V_t && H == 0), MGDP_E_INVALID, "V_t needs a finite horizon");
    return 0;
}

Geo eval_geo(const mgdp_vi *vi, const EvalShape &s) {
    Geo g = make_geo(vi);
    g.HWs = s.HWs;
    g.Ss = s.Ss;
    g.nbuf = 2;
    g.quad = g.pair = g.nmix = g.wt = 0;
    g.order = nullptr;
    g.kprio[0] = g.kprio[1] = g.kprio[2] = 0;
    return g;
}

int eval_buffers(mgdp_vi *vi) {
    if (!vi->d_eval) MGDP_HIP(hipMalloc((void **)&vi->d_eval, 2 * sizeof(unsigned long long)));
    return 0;
}

// A kernel of one workgroup per grid, timed: the LDS limit raised above 64 KiB, an event pair, the launch with
// eval_geo as its first argument and `args` behind it.  The caller reads the launch error.
template <typename K, typename... Args>
int launch_per_grid(mgdp_vi *vi, K kern, int block, int lds, Args... args) {
    const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
    if (lds > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    TimedPair tp;
    if (int rc = vi->timed.begin(-1, &tp)) return rc;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(block), lds, vi->stream, tp.a, tp.b, 0, eval_geo(vi, s), args...);
    return 0;
}
// ... on eval_shape's block and LDS (the evaluation kernels, the occupancy kernel)
template <typename K, typename... Args>
int launch_on_eval_shape(mgdp_vi *vi, K kern, Args... args) {
    const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
    return launch_per_grid(vi, kern, s.block, s.lds, args...);
}

// The launch of an evaluation kernel (vi_eval_kernel, vi_eval_nd_kernel, vi_eval_fh_kernel): the arguments
// the three share, the kernel's own (`tail`), then in_kernel_reduce and the epoch.
template <typename T, typename K, typename... Tail>
int launch_eval_kernel(mgdp_vi *vi, K kern, const int8_t *pi_src, Tail... tail) {
    if (int rc = launch_on_eval_shape(vi, kern, make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], pi_src, vi->d_pi, vi->d_kenv,
                                      vi->d_dvenv, vi->d_red, vi->d_ticket, vi->d_hout, vi->d_eval, tail...,
                                      vi->d.B <= vi->kn.inkernel_max ? 1 : 0, next_host_epoch(vi)))
        return rc;
    return after_grid_launch(vi, vi->d_hout, false);
}

// Dispatch on (dtype, model, slip, NoDeath lava); the mapping does not apply (one thread per cell).  DoorKey
// has neither slip nor NoDeath (mgdp_vi_create), so neither is instantiated.
template <typename T, template <typename, int, bool, bool> class F, typename... Args>
int dispatch_eval_t(mgdp_vi *vi, Args... args) {
    if (vi->d.model == MGDP_MODEL_DOORKEY) return F<T, MGDP_MODEL_DOORKEY, false, false>::run(vi, args...);
    return fan_out2(vi->d.slip_p >= 0.0, vi->d.lava_mode == MGDP_LAVA_NODEATH, [&](auto SLIP, auto ND) {
        return F<T, MGDP_MODEL_XYD, decltype(SLIP)::value, decltype(ND)::value>::run(vi, args...);
    });
}
template <template <typename, int, bool, bool> class F, typename... Args>
int dispatch_eval(mgdp_vi *vi, Args... args) {
    return vi->d.dtype == MGDP_F32 ? dispatch_eval_t<float, F>(vi, args...) : dispatch_eval_t<double, F>(vi, args...);
}

template <typename T, int MODEL, bool SLIP, bool ND>
struct EvalF {  // NoDeath lava: vi_eval_nd_kernel under the same protocol
    static int run(mgdp_vi *vi, int k_target, const int8_t *pi_src) {
        if constexpr (ND) return launch_eval_kernel<T>(vi, vi_eval_nd_kernel<T, SLIP>, pi_src, k_target, vi->fresh);
        else return launch_eval_kernel<T>(vi, vi_eval_kernel<T, MODEL, SLIP>, pi_src, k_target, vi->fresh);
    }
};
template <typename T, int MODEL, bool SLIP, bool ND>
struct EvalFhF {  // + (time-indexed policy, V_t stored)
    static int run(mgdp_vi *vi, const int8_t *pi_src, bool ti, void *d_vt) {
        const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
        constexpr int max_block = kEvalFhBlock<T, MODEL>;
        MGDP_CHECK(s.block <= max_block, MGDP_E_UNSUPPORTED, "policy evaluation: %d cell slots exceed the kernel's %d threads",
                   s.block, max_block);
        return fan_out2(ti, d_vt != nullptr, [&](auto TI, auto VT) {
            return launch_eval_kernel<T>(vi, vi_eval_fh_kernel<T, MODEL, SLIP, ND, decltype(TI)::value, decltype(VT)::value>, pi_src,
                                         (const T *)vi->d_rgoal, (T *)d_vt, vi->d.horizon);
        });
    }
};
template <typename T, int MODEL, bool SLIP, bool ND>
struct ImproveF {
    static int run(mgdp_vi *vi) {
        const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
        auto kern = vi_improve_kernel<T, MODEL, SLIP, ND>;
        if (s.improve_lds > 64 * 1024)
            MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, s.improve_lds));
        hipLaunchKernelGGL(kern, dim3(vi->d.B), dim3(s.improve_block), s.improve_lds, vi->stream, eval_geo(vi, s),
                           make_coef<T>(vi), vi->d_cells, (const T *)vi->d_V[0], vi->d_pi, vi->d_eval + 1);
        MGDP_HIP(hipGetLastError());
        return 0;
    }
};

// Before an evaluation's first launch, stream idle of servers.  The dispatch order a later solve would learn
// from the previous solve's executed sweeps is learned first: the evaluation overwrites d_kexec with its own
// and must not feed that order.
int eval_begin(mgdp_vi *vi) {
    if (learned_order_due(vi))
        if (int rc = learn_dispatch(vi)) return rc;
    if (int rc = eval_buffers(vi)) return rc;
    MGDP_HIP(hipMemsetAsync(vi->d_eval, 0xff, sizeof(unsigned long long), vi->stream));
    protocol_state_reset(vi);
    vi->evaluated = true;  // whatever follows, kenv / dvenv / V are no longer a solve's
    return 0;
}
// the policy error word the first launch left (kEvalNoError: every entry in range); drains the stream
int eval_error_word(mgdp_vi *vi, unsigned long long *err) {
    *err = kEvalNoError;
    MGDP_HIP(hipMemcpyAsync(err, vi->d_eval, sizeof(*err), hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    vi->k_done_valid = false;
    return 0;
}
// an evaluation ended at sweep k with dV(k) = dv: the handle's state, `converged` and the out-parameters
int eval_finish(mgdp_vi *vi, int32_t k, double dv, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    vi->k_done = k;
    vi->k_done_valid = false;  // the protocol entry points need a reset after an evaluation
    vi->sweeps = k;
    vi->converged = rule_report(vi->d.horizon, vi->d.tol, k, dv, sweeps_out, dv_out, converged_out);
    return 0;
}

// The discounted evaluation of the policy at d_src (device; the handle's own buffer included).
int eval_run(mgdp_vi *vi, const int8_t *d_src, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    if (int rc = eval_begin(vi)) return rc;
    int32_t k = 0, km = 0;
    double dv = 0.0;
    if (int rc = dispatch_eval<EvalF>(vi, -1, d_src)) return rc;
    if (int rc = reduce_env(vi, &k, &dv)) return rc;
    unsigned long long err;
    if (int rc = eval_error_word(vi, &err)) return rc;
    MGDP_CHECK(err == kEvalNoError, MGDP_E_INVALID, "policy: grid %d state %d: action %d is outside [0, %d)",
               (int)(err >> 32), (int)((err >> 8) & 0xffffffu), (int)(int8_t)(err & 0xffu), vi->A);
    // run_to(K): nothing to launch when every grid is at K or at an exact fixed point (mgdp_vi_run_to)
    if (!(vi->k_min == k || (vi->dv_red == 0.0 && vi->k_min > 0))) {
        if (int rc = dispatch_eval<EvalF>(vi, k, nullptr)) return rc;
        if (int rc = reduce_env(vi, &km, &dv)) return rc;
        MGDP_CHECK(km == k, MGDP_E_INVALID, "evaluate: run_to(%d) ended at sweep %d", k, km);
    }
    if (int rc = rule_sweeps(vi->d.tol, vi->d.max_sweeps, &k, &dv, [&](int32_t k1, double *d) {
            if (int e = dispatch_eval<EvalF>(vi, k1, nullptr)) return e;
            return reduce_env(vi, &km, d);
        }))
        return rc;
    return eval_finish(vi, k, dv, sweeps_out, dv_out, converged_out);
}

// The finite-horizon evaluation of the policy at d_src (T rows: 1 or H), one launch of exactly H sweeps.
int eval_fh_run(mgdp_vi *vi, const int8_t *d_src, int T, void *d_vt, int32_t *sweeps_out, double *dv_out,
                int32_t *converged_out) {
    const int H = vi->d.horizon;
    if (int rc = eval_begin(vi)) return rc;
    int32_t k = 0;
    double dv = 0.0;
    if (int rc = dispatch_eval<EvalFhF>(vi, d_src, T != 1, d_vt)) return rc;
    if (int rc = reduce_env(vi, &k, &dv)) return rc;
    unsigned long long err;
    if (int rc = eval_error_word(vi, &err)) return rc;
    if (err != kEvalNoError) {
        const int row = (int)((err >> kFhRowShift) & (unsigned long long)(kFhMaxH - 1));
        MGDP_CHECK(false, MGDP_E_INVALID, "policy: grid %d t %d state %d: action %d is outside [0, %d)",
                   (int)(err >> kFhGridShift), T == 1 ? 0 : H - 1 - row, (int)((err >> 8) & 0x3fffu),
                   (int)(int8_t)(err & 0xffu), vi->A);
    }
    MGDP_CHECK(k == H && vi->k_min == H, MGDP_E_INVALID, "evaluate: the horizon's %d sweeps ended at %d..%d", H, vi->k_min, k);
    return eval_finish(vi, k, dv, sweeps_out, dv_out, converged_out);  // a finite horizon is exact after H sweeps
}

int eval_policy(mgdp_vi *vi, const int8_t *d_src, int T, void *d_vt, int32_t *sweeps_out, double *dv_out,
                int32_t *converged_out) {
    if (vi->d.horizon == 0) return eval_run(vi, d_src, sweeps_out, dv_out, converged_out);
    return eval_fh_run(vi, d_src, T, d_vt, sweeps_out, dv_out, converged_out);
}

int improve_run(mgdp_vi *vi, int64_t *changed_out) {
    if (int rc = eval_buffers(vi)) return rc;
    MGDP_HIP(hipMemsetAsync(vi->d_eval + 1, 0, sizeof(unsigned long long), vi->stream));
    if (int rc = dispatch_eval<ImproveF>(vi)) return rc;
    unsigned long long n = 0;
    MGDP_HIP(hipMemcpyAsync(&n, vi->d_eval + 1, sizeof(n), hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    if (changed_out) *changed_out = (int64_t)n;
    return 0;
}

// ---- the four operations; `opts` as in eval_supported ----
int evaluate_device(mgdp_vi *vi, bool opts, const int8_t *d_pi, int T, void *d_vt, int32_t *sweeps_out, double *dv_out,
                    int32_t *converged_out) {
    if (int rc = eval_supported(vi, "policy evaluation", opts)) return rc;
    MGDP_CHECK((((uintptr_t)d_pi | (uintptr_t)d_vt) & 15u) == 0, MGDP_E_INVALID, "%s",
               option_handle(vi) ? "policy / V_t: the device pointers must be 16-byte aligned"
                                 : "policy: the device pointer must be 16-byte aligned");
    MGDP_CHECK(d_pi || T == 1 || vi->d_pi_t, MGDP_E_INVALID,
               "no per-step policy on the handle: create with MGDP_KEEP_POLICY_T, or pass pi");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const int8_t *src = d_pi ? d_pi : (T == 1 ? vi->d_pi : vi->d_pi_t);
    return eval_policy(vi, src, T, d_vt, sweeps_out, dv_out, converged_out);
}

int evaluate_host(mgdp_vi *vi, bool opts, const int8_t *pi, int T, void *V_t, int32_t *sweeps_out, double *dv_out,
                  int32_t *converged_out) {
    if (int rc = eval_supported(vi, "policy evaluation", opts)) return rc;
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const size_t BS = (size_t)vi->d.B * vi->S, HBS = (size_t)vi->d.horizon * BS;
    int8_t *dst = vi->d_pi;
    if (T != 1) {
        if (!vi->d_pi_stage) MGDP_HIP(hipMalloc((void **)&vi->d_pi_stage, HBS));
        dst = vi->d_pi_stage;
    }
    if (V_t && !vi->d_vt_stage) MGDP_HIP(hipMalloc(&vi->d_vt_stage, HBS * vi->tsize));
    MGDP_HIP(hipMemcpyAsync(dst, pi, (size_t)T * BS, hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));  // the caller's buffer is free when this returns
    if (int rc = eval_policy(vi, dst, T, V_t ? vi->d_vt_stage : nullptr, sweeps_out, dv_out, converged_out)) return rc;
    if (V_t) {
        MGDP_HIP(hipMemcpyAsync(V_t, vi->d_vt_stage, HBS * vi->tsize, hipMemcpyDeviceToHost, vi->stream));
        MGDP_HIP(hipStreamSynchronize(vi->stream));
    }
    return 0;
}

int improve(mgdp_vi *vi, bool opts, int64_t *changed_out) {
    if (int rc = greedy_supported(vi, "policy improvement", opts)) return rc;
    MGDP_CHECK(vi->sweeps > 0, MGDP_E_INVALID, "policy improvement: no value function (solve or evaluate first)");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    return improve_run(vi, changed_out);
}

int policy_iteration(mgdp_vi *vi, bool opts, const int8_t *pi0, int32_t max_iters, int32_t *iters_out,
                     int64_t *eval_sweeps_out, int64_t *changed_out, double *dv_out) {
    MGDP_CHECK(max_iters > 0, MGDP_E_INVALID, "max_iters must be > 0");
    if (int rc = greedy_supported(vi, "policy iteration", opts)) return rc;
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const size_t BS = (size_t)vi->d.B * vi->S;
    if (pi0) {
        MGDP_HIP(hipMemcpyAsync(vi->d_pi, pi0, BS, hipMemcpyHostToDevice, vi->stream));
        MGDP_HIP(hipStreamSynchronize(vi->stream));
    } else {  // "forward" everywhere; the evaluation stores -1 on absorbing states
        MGDP_HIP(hipMemsetAsync(vi->d_pi, 2, BS, vi->stream));
    }
    int32_t iters = 0, k = 0;
    int64_t total = 0, changed = 0;
    double dv = 0.0;
    do {
        if (int rc = eval_run(vi, vi->d_pi, &k, &dv, nullptr)) return rc;
        if (int rc = improve_run(vi, &changed)) return rc;
        total += k;
        ++iters;
    } while (changed != 0 && iters < max_iters);
    if (iters_out) *iters_out = iters;
    if (eval_sweeps_out) *eval_sweeps_out = total;
    if (changed_out) *changed_out = changed;
    if (dv_out) *dv_out = dv;
    return 0;
}

}  // namespace
