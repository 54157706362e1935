// vi_host_order.h -- the dispatch order of a batch, from the cells or from the last solve: set_order,
// order_eligible, learned_order_due, learn_dispatch (order_src 2), cells_dispatch (order_src 1) and what
// every cells load ends with (note_cells_loaded).
// Part of the single translation unit vi.hip: included after vi_host_serve.h.
#pragma once

namespace {

// Dispatch order (Geo::order / kprio): the grids ranked longest first in dispatch order (an LPT
// schedule: the launch's tail holds short grids, and at full residency every CU gets a stratified
// mix), and optionally (learn_prio) the top 1 / 10 / 50 % raise their waves' issue priority.  The
// key per grid is (order_src) 1 = its cells' depth proxy (vi_depth_kernel, computed at each cells
// load: the order holds from the first solve of fresh grids), 2 = the sweeps it executed in the
// previous solve (d_kexec; round 5's learned order, from the second solve on).  V, pi and the sweep
// counts never depend on it.
constexpr int kLearnMinB = 1024;
int set_order(mgdp_vi *vi, const std::vector<int32_t> &kx) {
    const int B = vi->d.B;
    std::vector<int32_t> idx(B);
    for (int i = 0; i < B; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return kx[a] > kx[b]; });
    if (!vi->d_order) MGDP_HIP(hipMalloc((void **)&vi->d_order, sizeof(int32_t) * (size_t)B));
    MGDP_HIP(hipMemcpyAsync(vi->d_order, idx.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    const int t1 = kx[idx[B / 100]], t10 = kx[idx[B / 10]], t50 = kx[idx[B / 2]];
    if (t50 > 0 && t1 > t50) {
        vi->kprio[0] = t1;
        vi->kprio[1] = std::max(t10, t50 + 1);
        vi->kprio[2] = t50 + 1;
    } else {
        vi->kprio[0] = vi->kprio[1] = vi->kprio[2] = 0;  // no spread to exploit
    }
    // mixed wave counts: the grids with keys >= mix_frac x the largest on two waves (they are the
    // first workgroups of the order just set)
    vi->nmix = 0;
    if ((vi->plan.kern == Loop::mix) && kx[idx[0]] > 0) {
        const int thr = std::max(1, (int)std::ceil(vi->kn.mix_frac * kx[idx[0]]));
        while (vi->nmix < B && kx[idx[vi->nmix]] >= thr) ++vi->nmix;
    }
    vi->order_valid = true;
    return 0;
}
bool order_eligible(const mgdp_vi *vi) {
    return vi->kn.order_src != 0 && (vi->kn.learn_order || vi->kn.learn_prio) && vi->d.B >= kLearnMinB &&
           vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts && !serve_eligible(vi);
}
// order_src 2: the order of the previous solve's executed sweeps has yet to be learned (mgdp_vi_reset,
// eval_begin: before anything overwrites d_kexec)
bool learned_order_due(const mgdp_vi *vi) {
    return !vi->order_valid && vi->kn.order_src == 2 && vi->solves_since_load > 0 && order_eligible(vi);
}
// order_src 2: from the executed sweeps of the previous solve
int learn_dispatch(mgdp_vi *vi) {
    std::vector<int32_t> kx(vi->d.B);
    MGDP_HIP(hipMemcpyAsync(kx.data(), vi->d_kexec, sizeof(int32_t) * (size_t)vi->d.B, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return set_order(vi, kx);
}
// order_src 1: from the cells just loaded (one small launch, a D2H copy of B words and a sort)
int cells_dispatch(mgdp_vi *vi) {
    if (!order_eligible(vi) || vi->kn.order_src != 1 || vi->HW > kDepthMaxHW) return 0;
    int32_t *d_depth = nullptr;
    MGDP_HIP(hipMallocAsync((void **)&d_depth, sizeof(int32_t) * (size_t)vi->d.B, vi->stream));
    hipLaunchKernelGGL(vi_depth_kernel, dim3(vi->d.B), dim3(64), 0, vi->stream, make_geo(vi),
                       (const uint8_t *)vi->d_cells, (int)vi->d.model, d_depth);
    hipError_t e = hipGetLastError();
    std::vector<int32_t> kx(vi->d.B);
    if (e == hipSuccess) e = hipMemcpyAsync(kx.data(), d_depth, sizeof(int32_t) * (size_t)vi->d.B, hipMemcpyDeviceToHost, vi->stream);
    if (e == hipSuccess) e = hipFreeAsync(d_depth, vi->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(vi->stream);
    if (e != hipSuccess) return hip_fail(e, "dispatch order from the cells", __FILE__, __LINE__);
    return set_order(vi, kx);
}
// New cells are in: handed to the resident server (the order and the solve count stand) or copied to d_cells.
int note_cells_loaded(mgdp_vi *vi, bool handed_off) {
    vi->cells_loaded = true;
    vi->k_done_valid = false;
    if (handed_off) return 0;
    vi->order_valid = false;
    vi->solves_since_load = 0;
    return cells_dispatch(vi);
}

}  // namespace
