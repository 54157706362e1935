// vi_host_qvalues.h -- the host path of the action-value read-out (vi_qvalues.h).  It reads
// the handle's V, cells and options and writes its two outputs only: V, pi, kenv, d_kexec, the protocol state
// and the dispatch order stay as they are.  Part of the single translation unit vi.hip: included after
// vi_host_eval.h (dispatch_eval, launch_per_grid, eval_supported).
#pragma once

namespace {

// exactly the handles mgdp_vi_improve_opts admits; a finite horizon in words of its own, first
int qvalues_supported(const mgdp_vi *vi) {
    MGDP_CHECK(vi->d.horizon == 0, MGDP_E_UNSUPPORTED,
               "action values are refused on a finite horizon: Q_t needs V_{t+1}, and the handle keeps V_0 only");
    if (int rc = eval_supported(vi, "action values", true)) return rc;
    MGDP_CHECK(vi->sweeps > 0, MGDP_E_INVALID, "action values: no value function (solve or evaluate first)");
    const int lds = qvalues_lds(vi->d.model, vi->HW, vi->HWp, vi->S, vi->tsize, true);
    MGDP_CHECK(lds <= 160 * 1024, MGDP_E_UNSUPPORTED, "action values: grid too large for the LDS staging (%d B > 160 KiB)", lds);
    return 0;
}

template <typename T, int MODEL, bool SLIP, bool ND>
struct QvaluesF {
    static int run(mgdp_vi *vi, void *d_Q, uint8_t *d_opt) {
        const int block = qvalues_block(vi->d.model, vi->HW);
        const int lds = qvalues_lds(vi->d.model, vi->HW, vi->HWp, vi->S, vi->tsize, d_Q != nullptr);
        if (int rc = launch_per_grid(vi, vi_qvalues_kernel<T, MODEL, SLIP, ND>, block, lds, make_coef<T>(vi), vi->d_cells,
                                     (const T *)vi->d_V[0], (T *)d_Q, d_opt))
            return rc;
        MGDP_HIP(hipGetLastError());
        return 0;
    }
};

// one launch on device pointers, complete on return
int qvalues_run(mgdp_vi *vi, void *d_Q, uint8_t *d_opt) {
    if (int rc = dispatch_eval<QvaluesF>(vi, d_Q, d_opt)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int action_values_device(mgdp_vi *vi, void *d_Q, uint8_t *d_opt) {
    MGDP_CHECK(d_Q || d_opt, MGDP_E_INVALID, "action values: both outputs are null");
    if (int rc = qvalues_supported(vi)) return rc;
    MGDP_CHECK((((uintptr_t)d_Q | (uintptr_t)d_opt) & 15u) == 0, MGDP_E_INVALID,
               "action values: the device pointers must be 16-byte aligned");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    return qvalues_run(vi, d_Q, d_opt);
}

int action_values_host(mgdp_vi *vi, void *Q, uint8_t *opt) {
    MGDP_CHECK(Q || opt, MGDP_E_INVALID, "action values: both outputs are null");
    if (int rc = qvalues_supported(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const size_t BS = (size_t)vi->d.B * vi->S;
    // staging: [0] Q, [1] opt, each grown at the first call that needs more
    const size_t need[2] = {Q ? BS * vi->A * vi->tsize : 0, opt ? BS : 0};
    for (int i = 0; i < 2; ++i) {
        if (need[i] <= vi->q_stage_cap[i]) continue;
        (void)hipFree(vi->d_q_stage[i]);
        vi->d_q_stage[i] = nullptr;
        vi->q_stage_cap[i] = 0;
        MGDP_HIP(hipMalloc(&vi->d_q_stage[i], need[i]));
        vi->q_stage_cap[i] = need[i];
    }
    if (int rc = qvalues_run(vi, Q ? vi->d_q_stage[0] : nullptr, opt ? (uint8_t *)vi->d_q_stage[1] : nullptr)) return rc;
    if (Q) MGDP_HIP(hipMemcpyAsync(Q, vi->d_q_stage[0], need[0], hipMemcpyDeviceToHost, vi->stream));
    if (opt) MGDP_HIP(hipMemcpyAsync(opt, vi->d_q_stage[1], need[1], hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

}  // namespace
