// vi_host_launch.h -- the launches of the solve's kernels and the plan's kernel pointers: launch_reduce
// and the tail every per-grid launch ends with (after_grid_launch); the option, fused, server and sweep
// launches; pick / Kernels / resolve_kernels (the plan's loops as kernel pointers); dispatch on (dtype,
// model, slip, mapping) with its ResolveF and SweepF, and fan_out2 for two run-time bools.  Part of the
// single translation unit vi.hip: included after vi_host.h.
#pragma once

namespace {

// {kmax, dV, kmin} of a launch too large to reduce in itself: kRedShards workgroups on the
// fused reduction's idle shards (MGDP_REDUCE_MULTI=0: the one-workgroup kernel)
inline void launch_reduce(mgdp_vi *vi, unsigned long long *pub) {
    if (vi->kn.reduce_multi)
        hipLaunchKernelGGL(vi_reduce_multi_kernel, dim3(kRedShards), dim3(256), 0, vi->stream, vi->d_kenv, vi->d_dvenv,
                           vi->d.B, vi->d_red, vi->d_ticket, pub, pub == vi->d_hout ? vi->epoch : 0u);
    else
        hipLaunchKernelGGL(vi_reduce_kernel, dim3(1), dim3(1024), 0, vi->stream, vi->d_kenv, vi->d_dvenv, vi->d.B,
                           pub, pub == vi->d_hout ? vi->epoch : 0u);
}

// After a launch of one workgroup per grid that publishes to `pub`: the launch error, V_0 consumed, and
// the reduce kernel where the batch is past inkernel_max and the launch did not reduce in itself.
inline int after_grid_launch(mgdp_vi *vi, unsigned long long *pub, bool reduced_in_launch) {
    MGDP_HIP(hipGetLastError());
    vi->fresh = 0;
    if (vi->d.B > vi->kn.inkernel_max && !reduced_in_launch) {
        launch_reduce(vi, pub);
        MGDP_HIP(hipGetLastError());
    }
    return 0;
}

template <typename T, int MODEL, bool SLIP, bool ND, int HMODE>
int launch_opts_t(mgdp_vi *vi, int k_target) {
    const Geo g = make_geo(vi);
    const Smem L = smem_layout(vi->plan.Ss, vi->HWp, sizeof(T), vi->plan.nbuf);
    auto kern = vi_fused_opts_kernel<T, MODEL, SLIP, ND, HMODE>;
    if (L.total() > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.total()));
    TimedPair tp;
    if (int rc = vi->timed.begin(-1, &tp)) return rc;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(vi->plan.block), L.total(), vi->stream, tp.a, tp.b, 0, g,
                          make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv, vi->d_dvenv,
                          vi->d_red, vi->d_ticket, vi->d_hout, k_target, vi->fresh,
                          vi->d.B <= vi->kn.inkernel_max ? 1 : 0, next_host_epoch(vi), (const T *)vi->d_rgoal, vi->d_pi_t);
    return after_grid_launch(vi, vi->d_hout, false);
}

// f(bool_constant<a>, bool_constant<b>): two run-time bools as template arguments of what f launches
template <typename F>
int fan_out2(bool a, bool b, F &&f) {
    if (a) return b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// runtime options -> template instantiation of the options kernel
template <typename T, int MODEL, bool SLIP, bool ND>
int launch_opts_h(mgdp_vi *vi, int k_target) {
    const int hm = vi->d.horizon > 0 ? ((vi->d.flags & MGDP_KEEP_POLICY_T) ? 2 : 1) : 0;
    if (hm == 2) return launch_opts_t<T, MODEL, SLIP, ND, 2>(vi, k_target);
    if (hm == 1) return launch_opts_t<T, MODEL, SLIP, ND, 1>(vi, k_target);
    return launch_opts_t<T, MODEL, SLIP, ND, 0>(vi, k_target);
}
template <typename T>
int launch_opts(mgdp_vi *vi, int k_target) {
    if (vi->d.model == MGDP_MODEL_DOORKEY) return launch_opts_h<T, MGDP_MODEL_DOORKEY, false, false>(vi, k_target);
    return fan_out2(vi->d.slip_p >= 0.0, vi->d.lava_mode == MGDP_LAVA_NODEATH, [&](auto SLIP, auto ND) {
        return launch_opts_h<T, MGDP_MODEL_XYD, decltype(SLIP)::value, decltype(ND)::value>(vi, k_target);
    });
}

// K<L, n>::fn for the run-time n among NS...; `dflt` if n is none of them.  The sequences below are
// exactly the sizes each family is compiled for.
template <template <Loop, int> class K, Loop L, typename F, int... NS>
F pick(int n, F dflt, std::integer_sequence<int, NS...>) {
    ((n == NS ? (void)(dflt = K<L, NS>::fn) : (void)0), ...);
    return dflt;
}
using N1to8 = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;  // wave2, band, dk_half and pair2 strides, bserve
using NWave = std::integer_sequence<int, 1, 2, 4, 8>;              // lone wave: cells per lane
using NMix = std::integer_sequence<int, 2, 3, 4, 5, 6>;            // mix (fp32)
using NWave2n = std::integer_sequence<int, 2, 3, 4>;               // wave2n: blocks per wave

template <typename T, int MODEL, bool SLIP, int MAP>
struct Kernels {
    template <Loop L, int N> struct Fused { static constexpr auto fn = vi_fused_kernel<T, MODEL, SLIP, MAP, L, N>; };
    template <Loop L, int N> struct Serve { static constexpr auto fn = vi_serve_kernel<T, MODEL, SLIP, MAP, L, N>; };
    template <Loop, int P> struct BServe { static constexpr auto fn = vi_bserve_kernel<T, P, false>; };
    template <Loop, int P> struct BServeMulti { static constexpr auto fn = vi_bserve_kernel<T, P, true>; };
};
// A kernel's signature depends on the value type alone: a launch casts the handle's pointer back.
template <typename T> using FusedFn = decltype(&vi_fused_kernel<T, MGDP_MODEL_XYD, false, MGDP_MAP_CELL>);
template <typename T> using ServeFn = decltype(&vi_serve_kernel<T, MGDP_MODEL_XYD, false, MGDP_MAP_CELL>);
template <typename T> using BServeFn = decltype(&vi_bserve_kernel<T, 1, false>);

// The plan's kernels.  A plan that names an instantiation this (dtype, model, slip, mapping) does not
// hold is an error, never another kernel.
template <typename T, int MODEL, bool SLIP, int MAP>
int resolve_kernels(const ViPlan &p, ViKernels *out) {
    using KS = Kernels<T, MODEL, SLIP, MAP>;
    FusedFn<T> f = KS::template Fused<Loop::generic, 0>::fn, own = nullptr;
    ServeFn<T> s = KS::template Serve<Loop::generic, 0>::fn;
    BServeFn<T> b = nullptr, bm = nullptr;
    bool f_ok = p.kern == Loop::generic, s_ok = p.serve_kern == Loop::generic;
    auto fused = [&](FusedFn<T> k) { f_ok = f_ok || k != f; f = k; };
    auto serve = [&](ServeFn<T> k) { s_ok = s_ok || k != s; s = k; };
    if constexpr (MAP == MGDP_MAP_CELL) {
        constexpr Loop soa = MODEL == MGDP_MODEL_XYD ? Loop::xyd_soa : Loop::dk_soa;
        if (p.kern == soa) fused(KS::template Fused<soa, 0>::fn);
    }
    if constexpr (MODEL == MGDP_MODEL_XYD && MAP == MGDP_MAP_CELL) {
        if (p.kern == Loop::wave) fused(pick<KS::template Fused, Loop::wave>(p.n, f, NWave{}));
        if (p.kern == Loop::xyd_x2) fused(KS::template Fused<Loop::xyd_x2, 0>::fn);
        if (p.kern == Loop::xyd_x4) fused(KS::template Fused<Loop::xyd_x4, 0>::fn);
        if (p.serve_kern == Loop::wave) serve(pick<KS::template Serve, Loop::wave>(p.serve_n, s, NWave{}));
        if (p.serve_kern == Loop::xyd_x2) serve(KS::template Serve<Loop::xyd_x2, 0>::fn);
        if constexpr (!SLIP) {
            if (p.kern == Loop::xyd_pair2) fused(pick<KS::template Fused, Loop::xyd_pair2>(p.n, f, N1to8{}));
            if (p.kern == Loop::wave2) fused(pick<KS::template Fused, Loop::wave2>(p.n, f, N1to8{}));
            if (p.kern == Loop::band) fused(pick<KS::template Fused, Loop::band>(p.n, f, N1to8{}));
            if (p.kern == Loop::wave2n) fused(pick<KS::template Fused, Loop::wave2n>(p.n, f, NWave2n{}));
            if constexpr (std::is_same<T, float>::value)
                if (p.kern == Loop::mix) fused(pick<KS::template Fused, Loop::mix>(p.n, f, NMix{}));
            if (p.serve_kern == Loop::serve_ew) serve(KS::template Serve<Loop::serve_ew, 0>::fn);
            if (p.serve_kern == Loop::serve_pair) serve(KS::template Serve<Loop::serve_pair, 0>::fn);
            if (p.serve_kern == Loop::band) serve(pick<KS::template Serve, Loop::band>(p.serve_n, s, N1to8{}));
            if (p.wants_bserve) {  // the wave2 loop of the same P (the capacity of both is the same by bserve_min_waves)
                b = pick<KS::template BServe, Loop::wave2>(p.wave2, b, N1to8{});
                bm = pick<KS::template BServeMulti, Loop::wave2>(p.wave2, bm, N1to8{});
            }
        }
    }
    if constexpr (MODEL == MGDP_MODEL_DOORKEY && MAP == MGDP_MAP_CELL && !SLIP) {
        if (p.kern == Loop::dk_1t) fused(KS::template Fused<Loop::dk_1t, 0>::fn);
        if (p.kern == Loop::dk_half) fused(pick<KS::template Fused, Loop::dk_half>(p.n, f, N1to8{}));
        if (p.kern == Loop::dk_rows) {
            fused(KS::template Fused<Loop::dk_rows, 0>::fn);
            // fp32 16x16 own-rule launches: the compile-time 256-thread variant
            if (sizeof(T) == 4 && p.HWs == 256 && p.block == 256) own = KS::template Fused<Loop::dk_rows16, 0>::fn;
        }
        if (p.serve_kern == Loop::dk_half) serve(pick<KS::template Serve, Loop::dk_half>(p.serve_n, s, N1to8{}));
    }
    MGDP_CHECK(f_ok && s_ok && (!p.wants_bserve || (b && bm)), MGDP_E_INVALID,
               "no kernel for the planned loop (%s size %d, served %s size %d)", name(p.kern, false), p.n,
               name(p.serve_kern, true), p.serve_n);
    out->to = (const void *)f;
    out->own = own ? (const void *)own : (const void *)f;
    out->serve = (const void *)s;
    out->bserve = (const void *)b;
    out->bserve_multi = (const void *)bm;
    return 0;
}

// pub: where the launch's {kmax, dV bits, kmin} go (default: the host-mapped words the host polls,
// epoch-tagged; the multi-GPU device protocol passes a device buffer it all-reduces, raw); k_dev: the target
// sweep read from device memory instead of k_target (mgdp_vi_run_to_dev).
template <typename T>
int launch_fused_t(mgdp_vi *vi, int k_target, unsigned long long *pub, const long long *k_dev, unsigned long long *mirror) {
    if (vi->plan.opts) return launch_opts<T>(vi, k_target);
    if (!pub) pub = vi->d_hout;
    const Geo g = make_geo(vi);
    const bool own_rule = k_target < 0 && !k_dev;
    const auto kern = reinterpret_cast<FusedFn<T>>(const_cast<void *>(own_rule ? vi->k.own : vi->k.to));
    const int block = vi->plan.block, smem = vi->plan.lds;
    static const bool debug_occ = std::getenv("MGDP_DEBUG_OCC") != nullptr;  // read once, not per launch
    if (debug_occ) {  // diagnostics: resident workgroups per CU of this launch
        int per_cu = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kern, block, smem);
        std::fprintf(stderr, "mgdp occupancy: %d workgroups/CU (block %d, LDS %d B)\n", per_cu, block, smem);
    }
    TimedPair tp;
    if (int rc = vi->timed.begin(-1, &tp)) return rc;
    // the in-launch reduction (GkCtx): a fresh own-rule launch of a resident one-wave batch folds
    // each grid's {k_e, dV at k_e} through the counter tree and publishes {kmax, dV, kmin} itself (no
    // reduce kernel); grids at an exact fixed point are complete for any K (fixed-point completion),
    // so run_to has nothing to launch unless some grid stopped with dV > 0
    unsigned long long *gk = (vi->plan.gk && own_rule && vi->fresh) ? vi->d_gk : nullptr;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(block), smem, vi->stream, tp.a, tp.b, 0, g,
                       make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv,
                       vi->d_dvenv, vi->d_red, vi->d_ticket, pub, k_target, vi->fresh,
                       vi->d.B <= vi->kn.inkernel_max ? 1 : 0, pub == vi->d_hout ? next_host_epoch(vi) : 0u, k_dev, mirror, gk);
    return after_grid_launch(vi, pub, gk != nullptr);  // a launch-wide-rule launch publishes its own reduction
}
int launch_fused(mgdp_vi *vi, int k_target, unsigned long long *pub = nullptr, const long long *k_dev = nullptr,
                 unsigned long long *mirror = nullptr) {
    return vi->d.dtype == MGDP_F32 ? launch_fused_t<float>(vi, k_target, pub, k_dev, mirror)
                                   : launch_fused_t<double>(vi, k_target, pub, k_dev, mirror);
}

// Launch the handle's server: the resident batch server (B > 1; bserve_eligible: a one-wave
// deterministic XYD batch) or the lone-grid server.
template <typename T>
int launch_serve_t(mgdp_vi *vi, unsigned int served) {
    const ViPlan &p = vi->plan;
    const bool batch = vi->d.B > 1;
    MGDP_CHECK(!batch || vi->k.bserve, MGDP_E_INVALID, "batch server: not a one-wave deterministic XYD batch");
    const Geo g = make_geo(vi);
    TimedPair tp;
    if (int rc = vi->timed.begin(-1, &tp)) return rc;
    account_server_clock(vi);  // a server that left on its own (idle / life limit) before this relaunch
    ++vi->serve_tag;
    if (batch) {
        static const bool force_multi = std::getenv("MGDP_BSERVE_FORCE_MULTI") != nullptr;  // diagnostics
        const bool multi = vi->d.B > p.bserve_cap || force_multi;
        const auto kern = reinterpret_cast<BServeFn<T>>(const_cast<void *>(multi ? vi->k.bserve_multi : vi->k.bserve));
        hipExtLaunchKernelGGL(kern, dim3(std::min(vi->d.B, p.bserve_cap)), dim3(64), p.lds, vi->stream, tp.a, tp.b, 0, g,
                              make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv, vi->d_dvenv, vi->d_hout,
                              vi->d_hout + kHoutReq, vi->d_breq, vi->d_gk, (unsigned long long)served, vi->serve_idle_ticks,
                              vi->serve_life_ticks, vi->serve_tag, vi->kn.bserve_copies, vi->kn.bserve_nap,
                              vi->kn.bserve_wait_pub,
                              vi->order_valid && vi->kn.learn_order ? (int)(vi->kn.bserve_prio_frac * vi->d.B) : 0);
    } else {
        const auto kern = reinterpret_cast<ServeFn<T>>(const_cast<void *>(vi->k.serve));
        hipExtLaunchKernelGGL(kern, dim3(1), dim3(p.block), p.serve_lds, vi->stream, tp.a, tp.b, 0, g,
                              make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv, vi->d_dvenv,
                              vi->d_hout, vi->d_hout + kHoutReq, (unsigned long long)served, vi->serve_idle_ticks,
                              vi->serve_life_ticks, vi->kn.serve_pollers, vi->serve_tag, vi->kn.serve_poll_dma,
                              vi->kn.serve_depth ? vi->kn.serve_depth_max : 0);
    }
    MGDP_HIP(hipGetLastError());
    return 0;
}
int launch_serve(mgdp_vi *vi, unsigned int served) {
    return vi->d.dtype == MGDP_F32 ? launch_serve_t<float>(vi, served) : launch_serve_t<double>(vi, served);
}

template <typename T, int MODEL, bool SLIP, int MAP, bool POLICY>
int launch_sweep_kernel(mgdp_vi *vi, const T *Vin, T *Vout, int k, int check_prev, TimedPair tp = {}) {
    const int m = vi->plan.sweep_m;
    const int smem = sweep_smem_bytes(vi->S, vi->HWp, sizeof(T), m);
    auto kern = vi_sweep_kernel<T, MODEL, SLIP, MAP, POLICY>;
    if (smem > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    const int groups = (vi->d.B + m - 1) / m;
    const int grid = std::min(groups, vi->plan.sweep_grid);
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(vi->plan.sweep_block), smem, vi->stream, tp.a, tp.b, 0, make_geo(vi), make_coef<T>(vi),
                       vi->d_cells, Vin, Vout, vi->d_pi, POLICY ? nullptr : vi->d_shards, k, check_prev, m);
    MGDP_HIP(hipGetLastError());
    return 0;
}

template <typename T, int MODEL, bool SLIP, int DEPTH>
int launch_sweep_pipe(mgdp_vi *vi, const T *Vin, T *Vout, int k, int check_prev, TimedPair tp) {
    const int smem = sweep_pipe_smem_bytes(vi->S, vi->HW, vi->plan.HWs, vi->HWp, sizeof(T));
    auto kern = vi_sweep_pipe_kernel<T, MODEL, SLIP, DEPTH>;
    if (smem > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    if (vi->pipe_grid == 0) {  // resident workgroups, at most 4 per CU
        // Empty-16 x 65536 (profiles/r06_sweep2/): 8 per CU (every resident slot, 2048 workgroups)
        // 98.5 us per sweep, 6 per CU 100.1, 5 94.4, 4 90.3-90.8 (6.10-6.13 TB/s compulsory), 3 92.5,
        // 2 109.3: four 256-thread workgroups, each with two grids' loads in flight, keep enough bytes
        // moving, and fewer co-resident workgroups contend less for the channels.
        int per_cu = 0, cus = 0;
        MGDP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kern, vi->plan.HWs, smem));
        MGDP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, vi->d.device));
        vi->pipe_grid = std::min(4, std::max(1, per_cu)) * std::max(1, cus);
        if (vi->kn.sweep_grid > 0) vi->pipe_grid = vi->kn.sweep_grid;
    }
    const int grid = std::min(vi->d.B, vi->pipe_grid);
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(vi->plan.HWs), smem, vi->stream, tp.a, tp.b, 0, make_geo(vi), make_coef<T>(vi),
                          vi->d_cells, Vin, Vout, vi->d_shards, k, check_prev);
    MGDP_HIP(hipGetLastError());
    return 0;
}

template <typename T, int MODEL, bool SLIP, int MAP>
int launch_sweep_t(mgdp_vi *vi, int k, int check_prev, bool policy) {
    const T *Vin = (const T *)vi->d_V[(k - 1) & 1];
    T *Vout = (T *)vi->d_V[k & 1];
    if (policy) return launch_sweep_kernel<T, MODEL, SLIP, MAP, true>(vi, Vin, Vout, k, 0);
    TimedPair tp;
    if (int rc = vi->timed.begin(k, &tp)) return rc;
    if constexpr (MAP == MGDP_MAP_CELL) {
        if (vi->plan.sweep_pipe == 1) return launch_sweep_pipe<T, MODEL, SLIP, 1>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 2) return launch_sweep_pipe<T, MODEL, SLIP, 2>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 3) return launch_sweep_pipe<T, MODEL, SLIP, 3>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 4) return launch_sweep_pipe<T, MODEL, SLIP, 4>(vi, Vin, Vout, k, check_prev, tp);
    }
    return launch_sweep_kernel<T, MODEL, SLIP, MAP, false>(vi, Vin, Vout, k, check_prev, tp);
}

// Dispatch on (dtype, model, slip, mapping).  DoorKey has no slip (mgdp_vi_create), so none is instantiated.
template <typename T, template <typename, int, bool, int> class F, typename... Args>
int dispatch_t(mgdp_vi *vi, Args... args) {
    const bool sa = vi->d.mapping == MGDP_MAP_SA;
    if (vi->d.model != MGDP_MODEL_XYD) return sa ? F<T, 1, false, 1>::run(vi, args...) : F<T, 1, false, 0>::run(vi, args...);
    if (vi->d.slip_p >= 0.0) return sa ? F<T, 0, true, 1>::run(vi, args...) : F<T, 0, true, 0>::run(vi, args...);
    return sa ? F<T, 0, false, 1>::run(vi, args...) : F<T, 0, false, 0>::run(vi, args...);
}
template <template <typename, int, bool, int> class F, typename... Args>
int dispatch(mgdp_vi *vi, Args... args) {
    return vi->d.dtype == MGDP_F32 ? dispatch_t<float, F>(vi, args...) : dispatch_t<double, F>(vi, args...);
}

template <typename T, int MODEL, bool SLIP, int MAP>
struct ResolveF {
    static int run(mgdp_vi *vi) { return resolve_kernels<T, MODEL, SLIP, MAP>(vi->plan, &vi->k); }
};
template <typename T, int MODEL, bool SLIP, int MAP>
struct SweepF {
    static int run(mgdp_vi *vi, int k, int check_prev, bool policy) {
        return launch_sweep_t<T, MODEL, SLIP, MAP>(vi, k, check_prev, policy);
    }
};

}  // namespace
