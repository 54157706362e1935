// vi.hip -- Jacobi value iteration over batches of Minigrid grids on MI355X (gfx950).
//
// DP semantics (DESIGN.md "A9"): the transition is MiniGridEnv.step, minigrid/minigrid_env.py:520-583
// (front_pos :392-419, DIR_TO_VEC minigrid/core/constants.py:49-58, cell predicates
// minigrid/core/world_object.py:46-64,114,129,142,165,178-195,244); the value-iteration rule is
// build-defined because the reference has none.  The CPU oracle
// (oracle/mgdp_oracle.c) states the same arithmetic in the same order; both are compiled with
// -ffp-contract=off so fp32 and fp64 results agree bit for bit.
//
// Data layout in HBM (one handle = B grids of W x H on one device):
//   cells  uint8  [B][HWp]      OBJECT_TO_IDX per cell, row-major y*W+x, padded to 16 B per grid
//   V      T      [2][B][S]     value double-buffer (fused method uses buffer 0 in place)
//   pi     int8   [B][S]        greedy action of the last sweep (-1 = absorbing state)
//   kenv   int32  [B], dvenv f64 [B]   sweeps done / last max|dV| per grid (fused method)
//   red    u64    [64][4] + u32 ticket fused-launch reduction (kmax, dV bits, kmin) -> host-mapped
//   shards u64    [max_sweeps][8]      per-sweep global max|dV| as f64 bits (sweep method),
//                                      8 atomic shards (blockIdx & 7) to spread contention
//
// Kernels (vi_kernels.h)
//   vi_fused_kernel   one workgroup per grid: cells + both V tiles + pi live in LDS for the
//                     whole solve; many sweeps per launch, one __syncthreads per sweep.
//   vi_serve_kernel   the same solve in a persistent workgroup serving lone-grid requests.
//   vi_fused_opts_kernel  the fused solve with NoDeath lava / finite horizon.
//   vi_sweep_kernel   one Jacobi sweep of every grid: per grid, V'[grid] is staged HBM->LDS (the
//                     LDS tile of the neighbourhood), updated from LDS, written back.
//   vi_eval_kernel / vi_improve_kernel (vi_eval.h)  policy evaluation under the same protocol, and the
//                     greedy improvement step.
//   vi_eval_fh_kernel / vi_eval_nd_kernel (vi_eval_opts.h)  the same under the handle options:
//                     finite-horizon backward induction of a stationary or time-indexed policy, and
//                     evaluation on NoDeath lava (the improvement there is vi_improve_kernel's ND
//                     form).
//   vi_occupancy_kernel (vi_occupancy.h)  the forward pass of a policy on the same options: state
//                     distribution, absorbed mass, discounted visitation and reward.
//   vi_qvalues_kernel (vi_qvalues.h)  the action values Q[B][S][A] of the handle's V and the set of maximising
//                     actions per state, one pass per grid.
// Device code is split into vi_model.h (model), vi_loops.h (workgroup loops), vi_kernels.h
// (kernels); the host side into vi_host.h (the handle), vi_host_launch.h (launches, the plan's kernel
// pointers), vi_host_serve.h (waits, resident servers, the solve's closing steps), vi_host_order.h
// (dispatch order), vi_host_eval.h, vi_host_occupancy.h and vi_host_qvalues.h (those host paths); this file
// holds the C ABI.
// Which loop a handle runs is decided once, in vi_plan.h (host-plain: plan_vi); vi_rule.h (host-plain)
// is the global stopping rule that closes every solve and evaluation; vi_layout.h holds the LDS sizes
// host and device share.
// Thread mappings (template MAP): MGDP_MAP_CELL = one thread per cell updating its 4 (XYD) or
// 16 (DoorKey) states from 16-B LDS vectors; MGDP_MAP_SA = one thread per (state, action),
// 8 lanes per state, wave shuffle max-reduce with the lowest action index winning ties.
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <climits>
#include <limits>
#include <type_traits>
#include <utility>
#include <cstring>
#include <vector>

#include "common.h"
#include "comm.h"
#include "timed.h"

#include "vi_plan.h"
#include "vi_rule.h"
#include "vi_model.h"
#include "vi_loops.h"
#include "vi_kernels.h"
#include "vi_eval.h"
#include "vi_eval_opts.h"
#include "vi_occupancy.h"
#include "vi_qvalues.h"

// ================================================================================================
// Host side
// ================================================================================================
using namespace mgdp;

#include "vi_host.h"
#include "vi_host_launch.h"
#include "vi_host_serve.h"
#include "vi_host_order.h"
#include "vi_host_eval.h"
#include "vi_host_occupancy.h"
#include "vi_host_qvalues.h"

extern "C" {

int mgdp_vi_num_states(const mgdp_vi_desc *d, int64_t *S) {
    MGDP_CHECK(d && S, MGDP_E_INVALID, "null argument");
    *S = (int64_t)d->W * d->H * (d->model == MGDP_MODEL_XYD ? 4 : 16);
    return 0;
}

int mgdp_vi_create(const mgdp_vi_desc *desc, mgdp_vi **out) {
    MGDP_CHECK(desc && out, MGDP_E_INVALID, "null argument");
    const mgdp_vi_desc &d = *desc;
    MGDP_CHECK(d.model == MGDP_MODEL_XYD || d.model == MGDP_MODEL_DOORKEY, MGDP_E_INVALID, "unknown model %d", d.model);
    MGDP_CHECK(d.dtype == MGDP_F32 || d.dtype == MGDP_F64, MGDP_E_INVALID, "unknown dtype %d", d.dtype);
    MGDP_CHECK(d.method == MGDP_METHOD_FUSED || d.method == MGDP_METHOD_SWEEP, MGDP_E_INVALID, "unknown method %d", d.method);
    MGDP_CHECK(d.mapping == MGDP_MAP_CELL || d.mapping == MGDP_MAP_SA, MGDP_E_INVALID, "unknown mapping %d", d.mapping);
    MGDP_CHECK(d.B > 0 && d.W >= 3 && d.H >= 3, MGDP_E_INVALID, "bad shape B=%d W=%d H=%d", d.B, d.W, d.H);
    MGDP_CHECK(d.max_sweeps > 0, MGDP_E_INVALID, "max_sweeps must be > 0");
    MGDP_CHECK(d.gamma >= 0.0 && (d.gamma < 1.0 || (d.horizon > 0 && d.gamma <= 1.0)), MGDP_E_INVALID,
               "gamma must be in [0, 1) (or [0, 1] with a finite horizon)");
    MGDP_CHECK(d.tol > 0.0, MGDP_E_INVALID, "tol must be > 0");
    MGDP_CHECK(!(d.slip_p >= 0.0 && d.model != MGDP_MODEL_XYD), MGDP_E_UNSUPPORTED,
               "slip transitions are defined for the XYD model only");
    MGDP_CHECK(d.slip_p <= 1.0, MGDP_E_INVALID, "slip_p must be <= 1");
    MGDP_CHECK(d.horizon >= 0, MGDP_E_INVALID, "horizon must be >= 0");
    MGDP_CHECK(d.lava_mode == MGDP_LAVA_TERMINAL || d.lava_mode == MGDP_LAVA_NODEATH, MGDP_E_INVALID,
               "unknown lava_mode %d", d.lava_mode);
    MGDP_CHECK(!(d.lava_mode == MGDP_LAVA_NODEATH && d.model != MGDP_MODEL_XYD), MGDP_E_UNSUPPORTED,
               "NoDeath lava is defined for the XYD model (DoorKey grids hold no lava)");
    MGDP_CHECK(!((d.flags & MGDP_KEEP_POLICY_T) && d.horizon == 0), MGDP_E_INVALID,
               "MGDP_KEEP_POLICY_T needs a finite horizon");
    MGDP_CHECK(!((d.horizon > 0 || d.lava_mode) && (d.method != MGDP_METHOD_FUSED || d.mapping != MGDP_MAP_CELL)),
               MGDP_E_UNSUPPORTED, "horizon / lava_mode options run on the fused MGDP_MAP_CELL path only");
    MGDP_CHECK(!(d.horizon > 0 && (long long)d.W * d.H > 1024), MGDP_E_UNSUPPORTED, "horizon needs W*H <= 1024");
    // the options kernel is strictly one thread per cell (fused_fast_xyd_soa) in a workgroup of <= 1024
    MGDP_CHECK(!(d.lava_mode == MGDP_LAVA_NODEATH && (long long)d.W * d.H > 1024), MGDP_E_UNSUPPORTED,
               "NoDeath lava needs W*H <= 1024");
    int ndev = 0;
    MGDP_HIP(hipGetDeviceCount(&ndev));
    MGDP_CHECK(d.device >= 0 && d.device < ndev, MGDP_E_HIP, "device %d not available (%d visible)", d.device, ndev);
    DeviceGuard guard(d.device);
    MGDP_CHECK(guard.ok, MGDP_E_HIP, "hipSetDevice(%d) failed", d.device);

    mgdp_vi *vi = new mgdp_vi();
    vi->d = d;
    vi->HW = d.W * d.H;
    vi->HWp = (int)round_up(vi->HW, 16);
    vi->S = vi->HW * (d.model == MGDP_MODEL_XYD ? 4 : 16);
    vi->A = d.model == MGDP_MODEL_XYD ? 7 : 5;
    vi->tsize = d.dtype == MGDP_F32 ? 4 : 8;
    // what runs: the knobs, the plan (vi_plan.h: the one place the variants' precedence is written),
    // its kernels, and the two numbers that need the device
    vi->kn = read_knobs();
    vi->plan = plan_vi(d, vi->kn);
    vi->serve_idle_ticks = (unsigned long long)vi->kn.serve_idle_us * 100ull;  // s_memrealtime ticks at 100 MHz
    vi->serve_life_ticks = (unsigned long long)vi->kn.serve_life_us * 100ull;
    const ViPlan &p = vi->plan;
    if (p.lds_base > 160 * 1024) {
        delete vi;
        set_error("grid too large for the LDS-resident kernels (%d B > 160 KiB)", p.lds_base);
        return MGDP_E_UNSUPPORTED;
    }
    if (int rc = dispatch<ResolveF>(vi)) {
        delete vi;
        return rc;
    }
    if (p.wants_gk) {  // resident workgroups of the one-wave launch and of the batch server running the same loop
        int cus = 0, fused_per_cu = 0, bserve_per_cu = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.device);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fused_per_cu, vi->k.to, p.block, p.lds) != hipSuccess) fused_per_cu = 0;
        if (p.wants_bserve && hipOccupancyMaxActiveBlocksPerMultiprocessor(&bserve_per_cu, vi->k.bserve, 64, p.lds) != hipSuccess)
            bserve_per_cu = 0;
        resolve_residency(vi->plan, fused_per_cu, bserve_per_cu, cus);
    }
    if (d.method == MGDP_METHOD_FUSED && !p.opts) {  // more than 64 KiB of LDS is opted into once per kernel
        hipError_t ea = hipSuccess;
        auto big = [&](const void *k, int lds) {
            if (ea == hipSuccess && lds > 64 * 1024) ea = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        };
        big(vi->k.own, p.lds);
        big(vi->k.to, p.lds);
        // (the pair server also holds the depth form's static level masks and table: vi_serve_depth.h)
        if (p.serve_shape) big(vi->k.serve, p.serve_lds + (p.serve_kern == Loop::serve_pair ? kDepthStaticLds : 0));
        if (ea != hipSuccess) {
            delete vi;
            return hip_fail(ea, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", __FILE__, __LINE__);
        }
    }

    const size_t BS = (size_t)d.B * vi->S;
    hipError_t e = hipSuccess;
    auto al = [&](void **p, size_t n) { if (e == hipSuccess) e = hipMalloc(p, n); };
    al((void **)&vi->d_cells, (size_t)d.B * vi->HWp);
    al(&vi->d_V[0], BS * vi->tsize);
    if (d.method == MGDP_METHOD_SWEEP) al(&vi->d_V[1], BS * vi->tsize);
    al((void **)&vi->d_pi, BS);
    al((void **)&vi->d_kenv, sizeof(int32_t) * d.B);
    al((void **)&vi->d_kexec, sizeof(int32_t) * d.B);
    if (e == hipSuccess) e = hipMemset(vi->d_kexec, 0, sizeof(int32_t) * d.B);
    al((void **)&vi->d_dvenv, sizeof(double) * d.B);
    al((void **)&vi->d_shards, sizeof(unsigned long long) * 8 * (size_t)(d.max_sweeps + 1));
    al((void **)&vi->d_red, sizeof(unsigned long long) * (kRedShards * 4 + 2));
    al((void **)&vi->d_pub1, sizeof(unsigned long long) * 4);
    if (vi->plan.gk || (vi->plan.bserve_cap > 0 && vi->plan.bserve_any)) {
        al((void **)&vi->d_gk, sizeof(unsigned long long) * gk_words(d.B));
        if (e == hipSuccess) e = hipMemset(vi->d_gk, 0, sizeof(unsigned long long) * gk_words(d.B));
    }
    if (vi->plan.bserve_cap > 0 && (d.B <= vi->plan.bserve_cap || vi->plan.bserve_any)) {
        al((void **)&vi->d_breq, sizeof(unsigned long long) * kBreqWords);
        if (e == hipSuccess) e = hipMemset(vi->d_breq, 0, sizeof(unsigned long long) * kBreqWords);
    }
    if (d.horizon > 0) {
        al(&vi->d_rgoal, (size_t)d.horizon * vi->tsize);
        if (d.flags & MGDP_KEEP_POLICY_T) al((void **)&vi->d_pi_t, (size_t)d.horizon * BS);
        if (e == hipSuccess) {  // goal reward of step_count t+1: _reward(), minigrid_env.py:235-240
            std::vector<unsigned char> rg((size_t)d.horizon * vi->tsize);
            for (int t = 0; t < d.horizon; ++t) {
                const double r = 1.0 - 0.9 * ((double)(t + 1) / (double)d.horizon);
                if (vi->tsize == 4) reinterpret_cast<float *>(rg.data())[t] = (float)r;
                else reinterpret_cast<double *>(rg.data())[t] = r;
            }
            e = hipMemcpy(vi->d_rgoal, rg.data(), rg.size(), hipMemcpyHostToDevice);
        }
    }
    if (e == hipSuccess) e = hipHostMalloc((void **)&vi->h_out, kHoutWords * sizeof(unsigned long long),
                                           hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&vi->d_hout, vi->h_out, 0);
    if (e == hipSuccess && d.B == 1) {
        e = hipHostMalloc((void **)&vi->h_stage, (size_t)vi->HWp, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&vi->d_stage, vi->h_stage, 0);
    }
    if (e == hipSuccess) {
        e = hipStreamCreateWithFlags(&vi->stream, hipStreamNonBlocking);
        vi->own_stream = e == hipSuccess;
    }
    if (e == hipSuccess) e = hipMemset(vi->d_cells, 0, (size_t)d.B * vi->HWp);
    if (vi->h_out) std::memset(vi->h_out, 0, kHoutWords * sizeof(unsigned long long));
    if (e == hipSuccess) {  // arm the fused reduction (every launch re-arms it for the next)
        std::vector<unsigned long long> init((size_t)kRedShards * 4 + 2, 0ull);
        for (size_t i = 2; i < (size_t)kRedShards * 4; i += 4) init[i] = 0x7fffffffull;
        e = hipMemcpy(vi->d_red, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
        vi->d_ticket = reinterpret_cast<unsigned int *>(vi->d_red + kRedShards * 4);
    }
    if (e != hipSuccess) {
        mgdp_vi_destroy(vi);
        return hip_fail(e, "mgdp_vi_create allocation", __FILE__, __LINE__);
    }
    *out = vi;
    return mgdp_vi_reset(vi);
}

int mgdp_vi_destroy(mgdp_vi *vi) {
    if (!vi) return 0;
    DeviceGuard guard(vi->d.device);
    (void)server_stop(vi);
    if (vi->stream) (void)hipStreamSynchronize(vi->stream);
    vi->timed.destroy();
    for (void *p : {(void *)vi->d_cells, vi->d_V[0], vi->d_V[1], (void *)vi->d_pi, (void *)vi->d_kenv, (void *)vi->d_kexec,
                    (void *)vi->d_order, (void *)vi->d_dvenv, (void *)vi->d_shards, (void *)vi->d_red, (void *)vi->d_pub1,
                    (void *)vi->d_gk, (void *)vi->d_breq, vi->d_rgoal, (void *)vi->d_pi_t, (void *)vi->d_eval,
                    (void *)vi->d_pi_stage, vi->d_vt_stage, (void *)vi->d_occ_err, vi->d_occ_tab})
        (void)hipFree(p);  // every device buffer of the handle (null where never allocated)
    for (void *p : vi->d_occ_stage) (void)hipFree(p);
    for (void *p : vi->d_q_stage) (void)hipFree(p);
    if (vi->h_out) (void)hipHostFree(vi->h_out);
    if (vi->h_stage) (void)hipHostFree(vi->h_stage);
    if (vi->own_stream) (void)hipStreamDestroy(vi->stream);
    delete vi;
    return 0;
}

int mgdp_vi_set_stream(mgdp_vi *vi, void *s) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = drain(vi)) return rc;
    if (vi->own_stream) { (void)hipStreamDestroy(vi->stream); vi->own_stream = false; vi->stream = nullptr; }
    if (s) {
        vi->stream = (hipStream_t)s;
    } else {
        MGDP_HIP(hipStreamCreateWithFlags(&vi->stream, hipStreamNonBlocking));
        vi->own_stream = true;
    }
    return 0;
}

int mgdp_vi_load_cells(mgdp_vi *vi, const uint8_t *cells) {
    MGDP_CHECK(vi && cells, MGDP_E_INVALID, "null argument");
    if (int rc = validate_cells(vi->d, cells)) return rc;
    // a resident lone-grid server takes the grid with its next request: staged in host memory
    // (a solve is synchronous, so the server is not reading the staging buffer now)
    if (vi->h_stage && vi->serving && serve_eligible(vi)) {
        std::memcpy(vi->h_stage, cells, vi->HW);
        if (serve_handoff(vi, vi->d_stage)) return note_cells_loaded(vi, true);
    }
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    std::vector<uint8_t> pad((size_t)vi->d.B * vi->HWp, 0);
    for (int b = 0; b < vi->d.B; ++b) std::memcpy(&pad[(size_t)b * vi->HWp], cells + (size_t)b * vi->HW, vi->HW);
    MGDP_HIP(hipMemcpyAsync(vi->d_cells, pad.data(), pad.size(), hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return note_cells_loaded(vi, false);
}

int mgdp_vi_load_cells_device(mgdp_vi *vi, const uint8_t *d_cells) {
    MGDP_CHECK(vi && d_cells, MGDP_E_INVALID, "null argument");
    // The resident server reads the bytes itself with its next request, unordered with respect to
    // any stream: only on the handle's own stream, where no caller kernel can still be producing
    // them.  On a caller-bound stream (mgdp_vi_set_stream) the copy below is ordered after whatever
    // the caller enqueued there before this call.
    if (vi->own_stream && serve_handoff(vi, d_cells)) return note_cells_loaded(vi, true);
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipMemcpy2DAsync(vi->d_cells, vi->HWp, d_cells, vi->HW, vi->HW, vi->d.B, hipMemcpyDeviceToDevice, vi->stream));
    return note_cells_loaded(vi, false);
}

int mgdp_vi_reset(mgdp_vi *vi) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (learned_order_due(vi)) {
        if (int rc = server_stop(vi)) return rc;
        if (int rc = learn_dispatch(vi)) return rc;
    }
    if (vi->d.method == MGDP_METHOD_SWEEP) {  // V_0 = 0 and an empty dV trace
        const size_t BS = (size_t)vi->d.B * vi->S;
        MGDP_HIP(hipMemsetAsync(vi->d_V[0], 0, BS * vi->tsize, vi->stream));
        MGDP_HIP(hipMemsetAsync(vi->d_shards, 0, sizeof(unsigned long long) * 8 * (size_t)(vi->d.max_sweeps + 1), vi->stream));
    }
    protocol_state_reset(vi);
    vi->evaluated = false;
    return 0;
}

int mgdp_vi_run_local(mgdp_vi *vi, int32_t *k_local_max) {
    MGDP_CHECK(vi && k_local_max, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    if (int rc = not_evaluated(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    if (vi->d.method == MGDP_METHOD_FUSED) {
        // the batch server only for mgdp_vi_solve's own run_local: a caller driving run_local / run_to
        // itself (a collective protocol) may enqueue device work between them that needs the CU slots a
        // resident batch server holds
        const bool serve = (serve_eligible(vi) || (vi->solving && bserve_eligible(vi))) && vi->fresh;
        if (serve) {
            if (int rc = serve_request(vi)) return rc;
        } else {
            if (int rc = server_stop(vi)) return rc;
            // a finite horizon is exactly H backward sweeps from V_H = 0
            if (vi->d.horizon > 0) MGDP_CHECK(vi->fresh, MGDP_E_INVALID, "finite horizon: call mgdp_vi_reset first");
            if (int rc = launch_fused(vi, vi->d.horizon > 0 ? vi->d.horizon : -1)) return rc;
        }
        int32_t km;
        if (int rc = reduce_env(vi, &km, nullptr)) return rc;
        if (serve) vi->serve_last = std::chrono::steady_clock::now();
        *k_local_max = km;
        return 0;
    }
    double dv = 0.0;
    if (int rc = sweep_run(vi, vi->d.max_sweeps, false, &dv)) return rc;
    vi->k_min = vi->k_max = vi->k_done;  // the sweep method stops the whole batch at once
    vi->dv_red = dv;
    vi->k_done_valid = true;
    *k_local_max = vi->k_done;
    return 0;
}

int mgdp_vi_run_to(mgdp_vi *vi, int32_t k_target, double *dv_out) {
    MGDP_CHECK(vi && dv_out, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(k_target >= 0 && k_target <= vi->d.max_sweeps, MGDP_E_INVALID, "k_target %d out of range", k_target);
    if (int rc = not_evaluated(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    if (vi->d.method == MGDP_METHOD_FUSED) {
        // every grid is already there: at k_target, or every grid at an exact fixed point (the
        // largest |dV| of the last launch is 0) at or below it -- fixed-point completion (fused_grid):
        // its V and pi are those of every later sweep, so no launch is needed
        const bool all_fixed = vi->dv_red == 0.0 && vi->k_min > 0 && vi->k_max <= k_target && vi->d.horizon == 0;
        if (vi->k_done_valid && (vi->k_min == k_target || all_fixed)) {
            vi->k_done = vi->k_min = vi->k_max = k_target;
            *dv_out = vi->dv_red;
            return 0;
        }
        MGDP_CHECK(vi->d.horizon == 0, MGDP_E_INVALID,
                   "finite horizon: the DP is exactly H sweeps (mgdp_vi_run_local / mgdp_vi_solve)");
        if (int rc = server_stop(vi)) return rc;
        if (int rc = launch_fused(vi, k_target)) return rc;
        int32_t km;
        if (int rc = reduce_env(vi, &km, dv_out)) return rc;
        MGDP_CHECK(km == k_target, MGDP_E_INVALID, "run_to(%d): a grid is already at sweep %d", k_target, km);
        vi->k_done = k_target;
        return 0;
    }
    MGDP_CHECK(k_target >= vi->k_done, MGDP_E_INVALID, "run_to(%d) behind sweep %d", k_target, vi->k_done);
    if (k_target == vi->k_done) {
        std::vector<unsigned long long> sh(8);
        if (k_target == 0) { *dv_out = 0.0; return 0; }
        MGDP_HIP(hipMemcpy(sh.data(), vi->d_shards + (long long)(k_target - 1) * 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        *dv_out = shard_max(sh.data());
        return 0;
    }
    return sweep_run(vi, k_target, true, dv_out);
}

// Multi-GPU device protocol (distributed.py): the two launches of a sharded solve are enqueued on
// the handle's stream with their results in a caller-owned device buffer, so the all-reduces
// between them (RCCL, ordered on the same stream) need no host round trip; the host reads K and dV
// once at the end and hands them back with mgdp_vi_set_result.
int mgdp_vi_run_local_dev(mgdp_vi *vi, int64_t *d_pub) {
    MGDP_CHECK(vi && d_pub, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    if (int rc = device_protocol_supported(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    vi->k_done_valid = false;
    return launch_fused(vi, -1, reinterpret_cast<unsigned long long *>(d_pub), (const long long *)nullptr);
}

int mgdp_vi_run_to_dev(mgdp_vi *vi, const int64_t *d_k, int64_t *d_pub) {
    MGDP_CHECK(vi && d_k && d_pub, MGDP_E_INVALID, "null argument");
    if (int rc = device_protocol_supported(vi)) return rc;
    MGDP_CHECK(!vi->fresh, MGDP_E_INVALID, "mgdp_vi_run_to_dev before mgdp_vi_run_local_dev");
    if (int rc = not_evaluated(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    vi->k_done_valid = false;
    return launch_fused(vi, 0, reinterpret_cast<unsigned long long *>(d_pub), reinterpret_cast<const long long *>(d_k));
}

int mgdp_vi_run_to_dev_sync(mgdp_vi *vi, const int64_t *d_kdv, int32_t *k_out, double *dv_out, double *dv_rule_out) {
    MGDP_CHECK(vi && d_kdv, MGDP_E_INVALID, "null argument");
    if (int rc = device_protocol_supported(vi)) return rc;
    MGDP_CHECK(!vi->fresh, MGDP_E_INVALID, "mgdp_vi_run_to_dev_sync before mgdp_vi_run_local_dev");
    if (int rc = not_evaluated(vi)) return rc;
    DeviceGuard guard(vi->d.device);
    vi->k_done_valid = false;
    int32_t km = 0;
    double dv = 0.0;
    // The gate (one wave): with E = d_kdv[1] == 0 every grid of every rank stopped its own rule at an
    // exact fixed point, so every grid is at K already (fixed-point completion) and the gate
    // publishes the result {K, dV 0}; else it publishes "more" and run_to(K) follows.  Either way
    // E goes to h_out[12..13] and the host waits on host-mapped words only.
    hipLaunchKernelGGL(vi_gate_kernel, dim3(1), dim3(64), 0, vi->stream, reinterpret_cast<const long long *>(d_kdv),
                       vi->d_hout, next_host_epoch(vi));
    MGDP_HIP(hipGetLastError());
    if (int rc = reduce_env(vi, &km, &dv)) return rc;
    if (vi->k_min != km) {
        // result -> host-mapped words (reduce_env polls them), d_kdv[1] -> h_out[12..13] by the launch
        if (int rc = launch_fused(vi, 0, (unsigned long long *)nullptr, reinterpret_cast<const long long *>(d_kdv),
                                      vi->d_hout + 12))
            return rc;
        if (int rc = reduce_env(vi, &km, &dv)) return rc;
    }
    MGDP_CHECK(vi->k_min == km, MGDP_E_INVALID, "run_to_dev_sync: grids ended at sweeps %d..%d, not at one common K",
               vi->k_min, km);
    vi->k_done = km;
    // the mirror's two tagged words were stored with the result's (no order between them)
    const volatile unsigned long long *h = vi->h_out;
    const unsigned long long ep = (unsigned long long)vi->epoch;
    for (uint64_t spin = 1; (h[12] >> 32) != ep || (h[13] >> 32) != ep; ++spin) {
        if ((spin & 1023u) == 0u) {
            const hipError_t q = hipStreamQuery(vi->stream);
            if (q == hipSuccess && ((h[12] >> 32) != ep || (h[13] >> 32) != ep))
                MGDP_CHECK(false, MGDP_E_HIP, "run_to_dev_sync: the launch finished without its E words (epoch %u)", vi->epoch);
            if (q != hipSuccess && q != hipErrorNotReady) return hip_fail(q, "run_to_dev_sync", __FILE__, __LINE__);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const unsigned long long rb = ((h[12] & 0xffffffffull) << 32) | (h[13] & 0xffffffffull);
    double rule;
    std::memcpy(&rule, &rb, sizeof(double));
    if (k_out) *k_out = km;
    if (dv_out) *dv_out = dv;
    if (dv_rule_out) *dv_rule_out = rule;
    return 0;
}

int mgdp_vi_local_result(const mgdp_vi *vi, int32_t *k_max, double *dv, int32_t *k_min) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(vi->k_done_valid, MGDP_E_INVALID, "no launch result to report (run mgdp_vi_run_local first)");
    if (k_max) *k_max = vi->k_max;
    if (dv) *dv = vi->dv_red;
    if (k_min) *k_min = vi->k_min;
    return 0;
}

int mgdp_vi_set_result(mgdp_vi *vi, int32_t k, double dv) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(k >= 0 && k <= vi->d.max_sweeps, MGDP_E_INVALID, "sweep %d out of range", k);
    vi->k_min = vi->k_max = vi->k_done = k;
    vi->dv_red = dv;
    vi->k_done_valid = true;
    return 0;
}

int mgdp_vi_sweep(mgdp_vi *vi, double *dv_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    if (int rc = not_evaluated(vi)) return rc;
    if (vi->d.method == MGDP_METHOD_FUSED) {
        MGDP_CHECK(vi->k_done_valid && vi->k_min == vi->k_max, MGDP_E_INVALID,
                   "mgdp_vi_sweep: grids are not at a common sweep index (call mgdp_vi_run_to first)");
        return mgdp_vi_run_to(vi, vi->k_max + 1, dv_out);
    }
    return mgdp_vi_run_to(vi, vi->k_done + 1, dv_out);
}

int mgdp_vi_finish(mgdp_vi *vi, int32_t sweeps) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    vi->sweeps = sweeps;
    if (vi->d.method == MGDP_METHOD_SWEEP && sweeps > 0) {
        MGDP_CHECK(sweeps == vi->k_done, MGDP_E_INVALID, "finish(%d) but %d sweeps were run", sweeps, vi->k_done);
        // pi of sweep k = argmax evaluated on V_{k-1} (bit-identical to what sweep k computed)
        if (int rc = dispatch<SweepF>(vi, sweeps, 0, true)) return rc;
        vi->cur = sweeps & 1;
        MGDP_HIP(hipStreamSynchronize(vi->stream));
    }
    // fused: V and pi were written by the launch whose result was already observed; later reads
    // (mgdp_vi_get_*) are ordered on the stream
    return 0;
}

// Served (solve_served: a request to the resident server)?  Else reset, launch, close (solve_close).
int mgdp_vi_solve(mgdp_vi *vi, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    bool served = false;
    const int rc_served = solve_served(vi, &served, sweeps_out, dv_out, converged_out);
    if (rc_served || served) return rc_served;
    DeviceGuard guard(vi->d.device);  // the entry points below nest inside it (no runtime call each)
    if (int rc = mgdp_vi_reset(vi)) return rc;
    int32_t k = 0;
    double dv = 0.0;
    // Deterministic batches take the plain path: their grids end their own rule at exact fixed
    // points, so run_local's result completes the solve (run_to launches nothing, see
    // mgdp_vi_run_to) -- one launch and one wait.  Slip batches keep the chained pair.
    if (vi->kn.chain && !vi->plan.gk && vi->d.slip_p >= 0.0 && vi->d.method == MGDP_METHOD_FUSED && vi->d.horizon == 0 &&
        !vi->plan.opts && !serve_eligible(vi)) {
        // The single-GPU form of the multi-GPU device protocol: run_local publishes {K, ...} to
        // device memory and run_to(K) reads K there, enqueued back to back -- no host round trip
        // and no launch gap between the two; the host waits once, for run_to's result.
        DeviceGuard guard(vi->d.device);
        if (int rc = server_stop(vi)) return rc;
        if (int rc = launch_fused(vi, -1, vi->d_pub1, (const long long *)nullptr)) return rc;
        if (int rc = launch_fused(vi, 0, (unsigned long long *)nullptr, (const long long *)vi->d_pub1)) return rc;
        if (int rc = reduce_env(vi, &k, &dv)) return rc;
        // run_to read K on the device: every grid must have ended exactly there (the host path's
        // km == k_target check)
        MGDP_CHECK(vi->k_min == k && vi->k_max == k, MGDP_E_INVALID,
                   "chained solve: grids ended at sweeps %d..%d, not at one common K", vi->k_min, vi->k_max);
        vi->k_done = k;
    } else {
        vi->solving = true;
        const int rc = mgdp_vi_run_local(vi, &k);
        vi->solving = false;
        if (rc) return rc;
        if (int rc2 = mgdp_vi_run_to(vi, k, &dv)) return rc2;
    }
    if (int rc = solve_close(vi, k, dv, sweeps_out, dv_out, converged_out)) return rc;
    ++vi->solves_since_load;
    return 0;
}

// The sharded solve with the library's own collectives (include/mgdp.h, ABI 11): the device
// protocol of distributed.py with RCCL called from here on the handle's stream instead of through
// torch.distributed -- run_local_dev publishes {K_r, E_r bits, kmin, 0} into the communicator's
// device words, ncclAllReduce(MAX) of the first two is enqueued right behind it, the gate (or
// run_to(K)) reads them on the device, and the host waits once on host-mapped words.  Only when
// some grid anywhere stopped its own rule with dV > 0 (E != 0: slip, rounding, a cap) is dV(K)
// all-reduced too, and only a rounding-level breach of the contraction runs fallback sweeps.
int mgdp_vi_solve_sharded(mgdp_vi *vi, mgdp_comm *comm, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi && comm, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts, MGDP_E_UNSUPPORTED,
               "the sharded solve runs the fused method without horizon / lava options");
    MGDP_CHECK(comm_device(comm) == vi->d.device, MGDP_E_INVALID, "communicator on device %d, handle on device %d",
               comm_device(comm), vi->d.device);
    DeviceGuard guard(vi->d.device);
    if (int rc = mgdp_vi_reset(vi)) return rc;
    int64_t *p = comm_proto(comm);
    if (int rc = mgdp_vi_run_local_dev(vi, p)) return rc;                  // {K_r, E_r bits, kmin, 0}
    if (int rc = comm_allreduce_max_dev(comm, p, 2, vi->stream)) return rc;  // {K, E} over every rank
    int32_t k = 0;
    double dv = 0.0, rule = 0.0;
    if (int rc = mgdp_vi_run_to_dev_sync(vi, p, &k, &dv, &rule)) return rc;  // the solve's one host wait
    comm_note_host_wait(comm);
    if (rule == 0.0) {
        // every grid of every rank stopped at an exact fixed point: dV at K is 0 everywhere
        MGDP_CHECK(dv == 0.0, MGDP_E_INVALID, "fixed-point invariant violated: dV at sweep %d is %g", k, dv);
    } else if (int rc = comm_max_double(comm, vi->stream, &dv)) {
        return rc;
    }
    if (int rc = mgdp_vi_set_result(vi, k, dv)) return rc;
    auto step = [vi, comm](int32_t, double *d) {  // a sweep of this rank's grids, then dV over every rank
        if (int rc = mgdp_vi_sweep(vi, d)) return rc;
        if (int rc = comm_max_double(comm, vi->stream, d)) return rc;
        vi->dv_red = *d;
        return 0;
    };
    if (int rc = solve_close(vi, k, dv, step, sweeps_out, dv_out, converged_out)) return rc;
    ++vi->solves_since_load;
    return 0;
}

// Checkpoint / resume (aux "checkpoint / resume"): Jacobi is memoryless given V_k,
// so a solve stopped at sweep k (a max_sweeps cap) continues from {V_k, k, dV_k} -- on this handle
// or on a new one in another process -- to the same global stopping sweep, V and pi, bit for bit,
// as the uninterrupted solve.  Every grid restarts its own rule at k (kenv / dvenv), then the
// batch is taken to the global K as in mgdp_vi_solve.  A converged checkpoint (dV < tol) has
// nothing left to do, and its pi (argmax on V_{k-1}) cannot be rebuilt from V_k: refused.
int mgdp_vi_resume(mgdp_vi *vi, const void *V, int32_t k, double dv, int32_t *sweeps_out, double *dv_out,
                   int32_t *converged_out) {
    MGDP_CHECK(vi && V, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    if (int rc = not_evaluated(vi)) return rc;
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && vi->d.horizon == 0, MGDP_E_INVALID,
               "resume: the fused method with an infinite horizon");
    MGDP_CHECK(k >= 1 && k < vi->d.max_sweeps, MGDP_E_INVALID, "resume: sweep %d outside [1, max_sweeps)", k);
    MGDP_CHECK(!(dv < vi->d.tol), MGDP_E_INVALID,
               "resume: the checkpoint has converged (dV %g < tol %g); its V and pi are final", dv, vi->d.tol);
    DeviceGuard guard(vi->d.device);
    // the copies below go through the null stream: drain the handle's own (or a caller-bound,
    // possibly non-blocking) stream first, so no earlier launch still reads V / kenv / dvenv
    if (int rc = drain(vi)) return rc;
    const size_t BS = (size_t)vi->d.B * vi->S;
    MGDP_HIP(hipMemcpy(vi->d_V[0], V, BS * vi->tsize, hipMemcpyHostToDevice));
    std::vector<int32_t> kk((size_t)vi->d.B, k);
    std::vector<double> dd((size_t)vi->d.B, dv);
    MGDP_HIP(hipMemcpy(vi->d_kenv, kk.data(), kk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MGDP_HIP(hipMemcpy(vi->d_kexec, kk.data(), kk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MGDP_HIP(hipMemcpy(vi->d_dvenv, dd.data(), dd.size() * sizeof(double), hipMemcpyHostToDevice));
    protocol_state_reset(vi);
    vi->fresh = 0;  // the next fused launch continues each grid from kenv / dvenv and V in HBM
    vi->k_done = vi->k_min = vi->sweeps = k;
    int32_t K = k;
    double dv2 = dv;
    if (int rc = mgdp_vi_run_local(vi, &K)) return rc;
    if (int rc = mgdp_vi_run_to(vi, K, &dv2)) return rc;
    return solve_close(vi, K, dv2, sweeps_out, dv_out, converged_out);
}

int mgdp_vi_evaluate_device(mgdp_vi *vi, const int8_t *d_pi, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return evaluate_device(vi, false, d_pi, 1, nullptr, sweeps_out, dv_out, converged_out);
}

int mgdp_vi_evaluate(mgdp_vi *vi, const int8_t *pi, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi && pi, MGDP_E_INVALID, "null argument");
    return evaluate_host(vi, false, pi, 1, nullptr, sweeps_out, dv_out, converged_out);
}

int mgdp_vi_improve(mgdp_vi *vi, int64_t *changed_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return improve(vi, false, changed_out);
}

int mgdp_vi_policy_iteration(mgdp_vi *vi, const int8_t *pi0, int32_t max_iters, int32_t *iters_out,
                             int64_t *eval_sweeps_out, int64_t *changed_out, double *dv_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return policy_iteration(vi, false, pi0, max_iters, iters_out, eval_sweeps_out, changed_out, dv_out);
}

int mgdp_vi_evaluate_opts_device(mgdp_vi *vi, const int8_t *d_pi, int32_t T, void *d_V_t, int32_t *sweeps_out,
                                 double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    if (int rc = eval_rows_supported(vi, T, d_V_t)) return rc;
    return evaluate_device(vi, true, d_pi, T, d_V_t, sweeps_out, dv_out, converged_out);
}

int mgdp_vi_evaluate_opts(mgdp_vi *vi, const int8_t *pi, int32_t T, void *V_t, int32_t *sweeps_out, double *dv_out,
                          int32_t *converged_out) {
    MGDP_CHECK(vi && pi, MGDP_E_INVALID, "null argument");
    if (int rc = eval_rows_supported(vi, T, V_t)) return rc;
    return evaluate_host(vi, true, pi, T, V_t, sweeps_out, dv_out, converged_out);
}

int mgdp_vi_improve_opts(mgdp_vi *vi, int64_t *changed_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return improve(vi, true, changed_out);
}

int mgdp_vi_policy_iteration_opts(mgdp_vi *vi, const int8_t *pi0, int32_t max_iters, int32_t *iters_out,
                                  int64_t *eval_sweeps_out, int64_t *changed_out, double *dv_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return policy_iteration(vi, true, pi0, max_iters, iters_out, eval_sweeps_out, changed_out, dv_out);
}

int mgdp_vi_occupancy_device(mgdp_vi *vi, const int8_t *d_pi, int32_t T, const int32_t *d_start, const void *d_mu0,
                             int32_t n_steps, void *d_mu, void *d_occ, void *d_ret, void *d_mu_t) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return occupancy_device(vi, d_pi, T, d_start, d_mu0, n_steps, d_mu, d_occ, d_ret, d_mu_t);
}

int mgdp_vi_occupancy(mgdp_vi *vi, const int8_t *pi, int32_t T, const int32_t *start, const void *mu0, int32_t n_steps,
                      void *mu, void *occ, void *ret, void *mu_t) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return occupancy_host(vi, pi, T, start, mu0, n_steps, mu, occ, ret, mu_t);
}

int mgdp_vi_action_values_device(mgdp_vi *vi, void *d_Q, uint8_t *d_opt) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return action_values_device(vi, d_Q, d_opt);
}

int mgdp_vi_action_values(mgdp_vi *vi, void *Q, uint8_t *opt) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    return action_values_host(vi, Q, opt);
}

int mgdp_vi_solve_last(mgdp_vi *vi, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    vi->last_req = true;
    const int rc = mgdp_vi_solve(vi, sweeps_out, dv_out, converged_out);
    vi->last_req = false;
    if (vi->serving) {  // the request carried kServeLast: the server is leaving (or already gone)
        vi->serving = false;
        vi->exiting = true;
    }
    return rc;
}

int mgdp_vi_persistent(const mgdp_vi *vi, int32_t *on) {
    MGDP_CHECK(vi && on, MGDP_E_INVALID, "null argument");
    *on = serve_eligible(vi) ? 1 : 0;
    return 0;
}

const char *mgdp_vi_kernel_name(const mgdp_vi *vi) {
    if (!vi) { set_error("null handle"); return nullptr; }
    return kernel_name(vi->plan, serve_eligible(vi));
}

const char *mgdp_vi_variant(const mgdp_vi *vi) {
    if (!vi) { set_error("null handle"); return nullptr; }
    return variant_name(vi->plan, serve_eligible(vi));
}

int mgdp_vi_get_values(mgdp_vi *vi, void *V) {
    MGDP_CHECK(vi && V, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    const void *src = vi->d.method == MGDP_METHOD_SWEEP ? vi->d_V[vi->cur] : vi->d_V[0];
    MGDP_HIP(hipMemcpyAsync(V, src, (size_t)vi->d.B * vi->S * vi->tsize, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int mgdp_vi_get_policy_t(mgdp_vi *vi, int8_t *pi_t) {
    MGDP_CHECK(vi && pi_t, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->d_pi_t, MGDP_E_INVALID, "no per-step policy: create with horizon > 0 and MGDP_KEEP_POLICY_T");
    DeviceGuard guard(vi->d.device);
    MGDP_HIP(hipMemcpyAsync(pi_t, vi->d_pi_t, (size_t)vi->d.horizon * vi->d.B * vi->S, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int mgdp_vi_get_policy(mgdp_vi *vi, int8_t *pi) {
    MGDP_CHECK(vi && pi, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipMemcpyAsync(pi, vi->d_pi, (size_t)vi->d.B * vi->S, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int mgdp_vi_get_grid_sweeps(mgdp_vi *vi, int32_t *k) {
    MGDP_CHECK(vi && k, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    if (vi->d.method == MGDP_METHOD_SWEEP) {
        std::fill(k, k + vi->d.B, (int32_t)vi->k_done);
        return 0;
    }
    MGDP_HIP(hipMemcpyAsync(k, vi->d_kexec, sizeof(int32_t) * (size_t)vi->d.B, hipMemcpyDeviceToHost, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int mgdp_vi_get_dv_trace(mgdp_vi *vi, double *trace, int32_t n) {
    MGDP_CHECK(vi && trace && n >= 0 && n <= vi->d.max_sweeps, MGDP_E_INVALID, "bad argument");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    std::vector<unsigned long long> sh((size_t)8 * n);
    if (n) MGDP_HIP(hipMemcpy(sh.data(), vi->d_shards, sh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) trace[i] = shard_max(&sh[8 * (size_t)i]);
    return 0;
}

int mgdp_vi_device_buffers(mgdp_vi *vi, void **d_V, void **d_pi) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    if (d_V) *d_V = vi->d.method == MGDP_METHOD_SWEEP ? vi->d_V[vi->cur] : vi->d_V[0];
    if (d_pi) *d_pi = vi->d_pi;
    return 0;
}

int mgdp_vi_synchronize(mgdp_vi *vi) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    // A resident server, or one leaving after its last request (mgdp_vi_solve_last), is the stream's
    // last work while nothing else was enqueued since (every other enqueue goes through server_stop
    // or a relaunch, which clear `exiting`): its tagged exit word then means the stream is done.
    if (vi->serving && !vi->pending_src) return server_stop(vi, false);
    if (vi->exiting && !vi->pending_src) {
        if (int rc = wait_server_exit(vi)) return rc;
        vi->exiting = false;
        return 0;
    }
    return drain(vi);
}

int mgdp_vi_enable_timing(mgdp_vi *vi, int32_t on) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = drain(vi)) return rc;
    if (int rc = vi->timed.restart(on != 0)) return rc;
    vi->clk_cycles = vi->clk_ticks = vi->clk_busy = vi->clk_solves = 0.0;
    vi->clk_launches = 0;
    return 0;
}

int mgdp_vi_serve_clock(mgdp_vi *vi, double *sclk_mhz, double *server_us, int64_t *launches, double *solve_us,
                        int64_t *solves) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    account_server_clock(vi);
    if (sclk_mhz) *sclk_mhz = vi->clk_ticks > 0 ? vi->clk_cycles / (vi->clk_ticks * 0.01) : 0.0;
    if (server_us) *server_us = vi->clk_ticks * 0.01;
    if (launches) *launches = vi->clk_launches;
    if (solve_us) *solve_us = vi->clk_solves > 0 ? vi->clk_busy * 0.01 / vi->clk_solves : 0.0;
    if (solves) *solves = (int64_t)vi->clk_solves;
    return 0;
}

int mgdp_vi_serve_path(mgdp_vi *vi, int32_t *path, int64_t *counts) {
    MGDP_CHECK(vi && path, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(vi->d.device);
    if (int rc = drain(vi)) return rc;  // the server writes the words behind its publish: it has left now
    account_server_clock(vi);
    *path = (int32_t)vi->h_out[kHoutPath];
    if (counts)
        for (int i = 0; i < 3; ++i) counts[i] = (int64_t)vi->path_counts[i];
    return 0;
}

int mgdp_vi_kernel_time(mgdp_vi *vi, double *total_ms, int64_t *launches) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = drain(vi)) return rc;
    return vi->timed.read(total_ms, launches);
}

}  // extern "C"
