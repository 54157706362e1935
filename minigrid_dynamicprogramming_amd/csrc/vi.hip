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
// Device code is split into vi_model.h (model), vi_loops.h (workgroup loops), vi_kernels.h
// (kernels); this file holds the host side and the C ABI.  Which loop a handle runs is decided once,
// in vi_plan.h (host-plain: plan_vi); vi_layout.h holds the LDS sizes host and device share.
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

#include "vi_plan.h"
#include "vi_model.h"
#include "vi_loops.h"
#include "vi_kernels.h"
#include "vi_eval.h"
#include "vi_eval_opts.h"
#include "vi_occupancy.h"


// ================================================================================================
// Host side
// ================================================================================================
using namespace mgdp;

// The kernels a plan names (resolve_kernels), type-erased: the fused own-rule and run-to launches
// (they differ for Loop::dk_rows16 only), the lone-grid server, the batch server resident / past
// its capacity (null unless the plan wants one).
struct ViKernels {
    const void *own = nullptr, *to = nullptr, *serve = nullptr, *bserve = nullptr, *bserve_multi = nullptr;
};

struct mgdp_vi {
    mgdp_vi_desc d;
    int S = 0, HW = 0, HWp = 0, A = 0, tsize = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint8_t *d_cells = nullptr;
    void *d_V[2] = {nullptr, nullptr};
    int8_t *d_pi = nullptr;
    int32_t *d_kenv = nullptr;
    int32_t *d_kexec = nullptr;  // per grid: the sweep it last computed (fixed-point grids keep theirs)
    int32_t *d_order = nullptr;  // dispatch order (Geo::order / kprio), from the cells at load or the last solve's d_kexec
    bool order_valid = false;
    int solves_since_load = 0;
    int kprio[3] = {0, 0, 0};
    double *d_dvenv = nullptr;
    unsigned long long *d_shards = nullptr;
    unsigned long long *d_red = nullptr;    // fused reduction shards [64][4]
    unsigned long long *d_pub1 = nullptr;   // device copy of a run_local launch's {kmax, dV, kmin, 0} (chained solve)
    unsigned int *d_ticket = nullptr;       // arrival ticket of the fused reduction
    // host-mapped words (kHoutWords): [0..3] {kmax, dV hi, dV lo, kmin} of a launch (each tagged with
    // its epoch), [5..7] the server's tagged result, [8..9] trace stamps, [11] server exit word,
    // [12..13] the run_to mirror (tagged),
    // [16] request word and [17] its source word (their own 128-B line: the server polls the pair)
    unsigned long long *h_out = nullptr;
    unsigned long long *d_hout = nullptr;   // device alias of h_out
    int cur = 0;        // V buffer holding the current V (sweep method)
    int k_min = 0;      // min / max sweeps over grids after the last reduce (fused method)
    int k_max = 0;
    bool k_done_valid = false;  // k_min / dv_red describe the current device state
    double dv_red = 0.0;
    int k_done = 0;     // sweeps completed by every grid (uniform after run_to / sweep)
    int32_t sweeps = 0, converged = 0;
    bool cells_loaded = false;
    // timing of the dominant kernel
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev, ev_pool;
    std::vector<int> ev_sweep;  // sweep index of each timed sweep launch (-1 = fused launch)
    double total_ms = 0.0;
    int64_t launches = 0;
    int fresh = 1;          // next fused launch starts from V_0 = 0
    unsigned int epoch = 0; // tag of the last fused launch; its result lands in h_out[0..3]
    // what runs (vi_plan.h): the MGDP_* knobs, the plan made of them at create, the plan's kernels
    ViKnobs kn;
    ViPlan plan;
    ViKernels k;
    int nmix = 0;                 // Loop::mix: the long grids (kexec >= mix_frac x the longest), set with the order
    int pipe_grid = 0;            // the pipelined sweep's grid: resident workgroups (set at the first launch)
    void *d_rgoal = nullptr;      // T[H]: the exact _reward() of step_count t+1, per t
    int8_t *d_pi_t = nullptr;     // int8[H][B][S] with MGDP_KEEP_POLICY_T
    // persistent solver (lone grid, fused one-thread-per-cell path): see vi_serve_kernel
    bool serving = false;         // a vi_serve_kernel launch may be resident on `stream`
    // The server leaves after serve_idle_ticks without a request, which also bounds how long a
    // device-wide synchronisation by another component can wait on it.
    unsigned long long serve_idle_ticks = 10000;     // 100 us at 100 MHz
    unsigned long long serve_life_ticks = 200000000; // 2 s
    std::chrono::steady_clock::time_point serve_last{};  // host time of the last served result
    // A new lone grid for a resident server: the bytes wait at pending_src (host-mapped staging
    // h_stage, or the caller's device memory) and the next request carries kServeNewCells; a server
    // stop before that copies them into d_cells instead.
    uint8_t *h_stage = nullptr;   // pinned, mapped: W*H bytes (B == 1 handles)
    uint8_t *d_stage = nullptr;   // its device alias
    unsigned long long pending_src = 0;
    bool last_req = false;        // the request being posted is the server's last (mgdp_vi_solve_last)
    bool exiting = false;         // a server told to leave after its last request is the stream's last work
    unsigned long long serve_tag = 0;  // tag of the latest server launch: its exit word (h_out[11]) carries it
    // clock of the departed servers since enable_timing (mgdp_vi_serve_clock): shader-clock cycles and
    // 100 MHz ticks of their lives, summed as each one's exit word is seen (kHoutClk)
    unsigned long long clk_tag = 0;  // the last server launch whose clock words were added
    double clk_cycles = 0.0, clk_ticks = 0.0, clk_busy = 0.0, clk_solves = 0.0;
    long long clk_launches = 0;
    long long path_counts[3] = {0, 0, 0};  // served requests of the departed pair servers by path (mgdp_vi_serve_path)
    unsigned long long *d_gk = nullptr;   // the in-launch reduction's device words (GkCtx; plan.gk)
    unsigned long long *d_breq = nullptr;  // the resident batch server's device words (kBreqWords): forwarded request, exit counter
    bool solving = false;                // inside mgdp_vi_solve: its run_local may use the batch server
    // policy evaluation / improvement (vi_eval.h): {policy error word, changed-state count}, allocated
    // at the first evaluation; `evaluated`: kenv / dvenv / V are an evaluation's (cleared by mgdp_vi_reset)
    unsigned long long *d_eval = nullptr;
    bool evaluated = false;
    // mgdp_vi_evaluate_opts (vi_eval_opts.h): device staging of a host time-indexed policy [H][B][S] and
    // of the host V_t output T [H][B][S], allocated at the first call that needs them
    int8_t *d_pi_stage = nullptr;
    void *d_vt_stage = nullptr;
    // mgdp_vi_occupancy (vi_occupancy.h): {policy error word, start error word}; the step tables T [3][N]
    // (disc, wg, wl) of the last N; device staging of the host form's policy, start / mu0, the three planes
    // and mu_t, each grown at the first call that needs more
    unsigned long long *d_occ_err = nullptr;
    void *d_occ_tab = nullptr;
    int occ_tab_n = 0;
    void *d_occ_stage[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t occ_stage_cap[4] = {0, 0, 0, 0};
};

namespace {

Geo make_geo(const mgdp_vi *vi) {
    Geo g;
    g.B = vi->d.B;
    g.W = vi->d.W;
    g.H = vi->d.H;
    g.HW = vi->HW;
    g.HWp = vi->HWp;
    g.HWs = vi->plan.HWs;
    g.Ss = vi->plan.Ss;
    g.S = vi->S;
    g.off[0] = 1;
    g.off[1] = vi->d.W;
    g.off[2] = -1;
    g.off[3] = -vi->d.W;
    g.max_sweeps = vi->d.max_sweeps;
    g.nbuf = vi->plan.nbuf;
    g.quad = vi->plan.quad;
    g.pair = vi->plan.pair;
    g.tol = vi->d.tol;
    g.kexec = vi->d_kexec;
    g.order = vi->order_valid && vi->kn.learn_order ? vi->d_order : nullptr;
    for (int i = 0; i < 3; ++i) g.kprio[i] = vi->order_valid && vi->kn.learn_prio ? vi->kprio[i] : 0;
    g.nmix = g.order && (vi->plan.kern == Loop::mix) ? vi->nmix : 0;
    g.wt = vi->plan.wt;
    return g;
}

template <typename T>
Coef<T> make_coef(const mgdp_vi *vi) {
    Coef<T> c;
    c.g = (T)vi->d.gamma;
    const double p = vi->d.slip_p;
    c.p = (T)p;
    c.c = (T)((1.0 - p) / 6.0);
    T t = (T)vi->d.tol;
    if ((double)t < vi->d.tol) t = std::nextafter(t, std::numeric_limits<T>::infinity());
    c.tol = t;
    c.dc = (T)vi->d.death_cost;
    return c;
}

// Timed launches go through hipExtLaunchKernelGGL with a start/stop event pair, so the events carry
// the dispatch's own begin/end timestamps (what rocprofv3's kernel trace reports) rather than the
// times of separate marker packets.  Event pairs are pooled: no hipEventCreate in the timed loop.
struct TimedPair { hipEvent_t a = nullptr, b = nullptr; };
int timed_begin(mgdp_vi *vi, int sweep_idx, TimedPair *tp) {
    tp->a = tp->b = nullptr;
    if (!vi->timing) return 0;
    std::pair<hipEvent_t, hipEvent_t> e;
    if (!vi->ev_pool.empty()) {
        e = vi->ev_pool.back();
        vi->ev_pool.pop_back();
    } else {
        MGDP_HIP(hipEventCreate(&e.first));
        MGDP_HIP(hipEventCreate(&e.second));
    }
    vi->ev.push_back(e);
    vi->ev_sweep.push_back(sweep_idx);
    tp->a = e.first;
    tp->b = e.second;
    return 0;
}
// Fold completed events into total_ms (called after a stream sync).  Sweep launches past the
// stopping sweep no-op and were marked uncounted (ev_sweep = INT_MAX) by sweep_run.
int timed_collect(mgdp_vi *vi) {
    for (size_t i = 0; i < vi->ev.size(); ++i) {
        if (vi->ev_sweep[i] != INT32_MAX) {
            float ms = 0.f;
            MGDP_HIP(hipEventElapsedTime(&ms, vi->ev[i].first, vi->ev[i].second));
            vi->total_ms += ms;
            vi->launches += 1;
        }
        vi->ev_pool.push_back(vi->ev[i]);
    }
    vi->ev.clear();
    vi->ev_sweep.clear();
    return 0;
}

// {kmax, dV, kmin} of a launch too large to reduce in itself: kRedShards workgroups on the
// fused reduction's idle shards (MGDP_REDUCE_MULTI=0: the one-workgroup kernel)
// The epoch of a launch whose result goes to the host-mapped words (never 0: publish() writes a
// device buffer's raw words for epoch 0)
inline unsigned int next_host_epoch(mgdp_vi *vi) {
    if (++vi->epoch == 0u) ++vi->epoch;
    return vi->epoch;
}

inline void launch_reduce(mgdp_vi *vi, unsigned long long *pub) {
    if (vi->kn.reduce_multi)
        hipLaunchKernelGGL(vi_reduce_multi_kernel, dim3(kRedShards), dim3(256), 0, vi->stream, vi->d_kenv, vi->d_dvenv,
                           vi->d.B, vi->d_red, vi->d_ticket, pub, pub == vi->d_hout ? vi->epoch : 0u);
    else
        hipLaunchKernelGGL(vi_reduce_kernel, dim3(1), dim3(1024), 0, vi->stream, vi->d_kenv, vi->d_dvenv, vi->d.B,
                           pub, pub == vi->d_hout ? vi->epoch : 0u);
}

template <typename T, int MODEL, bool SLIP, bool ND, int HMODE>
int launch_opts_t(mgdp_vi *vi, int k_target) {
    const Geo g = make_geo(vi);
    const Smem L = smem_layout(vi->plan.Ss, vi->HWp, sizeof(T), vi->plan.nbuf);
    auto kern = vi_fused_opts_kernel<T, MODEL, SLIP, ND, HMODE>;
    if (L.total() > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.total()));
    TimedPair tp;
    if (int rc = timed_begin(vi, -1, &tp)) return rc;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(vi->plan.block), L.total(), vi->stream, tp.a, tp.b, 0, g,
                          make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv, vi->d_dvenv,
                          vi->d_red, vi->d_ticket, vi->d_hout, k_target, vi->fresh,
                          vi->d.B <= vi->kn.inkernel_max ? 1 : 0, next_host_epoch(vi), (const T *)vi->d_rgoal, vi->d_pi_t);
    MGDP_HIP(hipGetLastError());
    vi->fresh = 0;
    if (vi->d.B > vi->kn.inkernel_max) {
        launch_reduce(vi, vi->d_hout);
        MGDP_HIP(hipGetLastError());
    }
    return 0;
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
    const bool slip = vi->d.slip_p >= 0.0, nd = vi->d.lava_mode == MGDP_LAVA_NODEATH;
    if (slip) return nd ? launch_opts_h<T, MGDP_MODEL_XYD, true, true>(vi, k_target)
                        : launch_opts_h<T, MGDP_MODEL_XYD, true, false>(vi, k_target);
    return nd ? launch_opts_h<T, MGDP_MODEL_XYD, false, true>(vi, k_target)
              : launch_opts_h<T, MGDP_MODEL_XYD, false, false>(vi, k_target);
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
    if (int rc = timed_begin(vi, -1, &tp)) return rc;
    // the in-launch reduction (GkCtx): a fresh own-rule launch of a resident one-wave batch folds
    // each grid's {k_e, dV at k_e} through the counter tree and publishes {kmax, dV, kmin} itself (no
    // reduce kernel); grids at an exact fixed point are complete for any K (fixed-point completion),
    // so run_to has nothing to launch unless some grid stopped with dV > 0
    unsigned long long *gk = (vi->plan.gk && own_rule && vi->fresh) ? vi->d_gk : nullptr;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(block), smem, vi->stream, tp.a, tp.b, 0, g,
                       make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], vi->d_pi, vi->d_kenv,
                       vi->d_dvenv, vi->d_red, vi->d_ticket, pub, k_target, vi->fresh,
                       vi->d.B <= vi->kn.inkernel_max ? 1 : 0, pub == vi->d_hout ? next_host_epoch(vi) : 0u, k_dev, mirror, gk);
    MGDP_HIP(hipGetLastError());
    vi->fresh = 0;
    if (vi->d.B > vi->kn.inkernel_max && !gk) {  // a launch-wide-rule launch publishes its own reduction
        launch_reduce(vi, pub);
        MGDP_HIP(hipGetLastError());
    }
    return 0;
}
int launch_fused(mgdp_vi *vi, int k_target, unsigned long long *pub = nullptr, const long long *k_dev = nullptr,
                 unsigned long long *mirror = nullptr) {
    return vi->d.dtype == MGDP_F32 ? launch_fused_t<float>(vi, k_target, pub, k_dev, mirror)
                                   : launch_fused_t<double>(vi, k_target, pub, k_dev, mirror);
}

void account_server_clock(mgdp_vi *vi);

// Launch the handle's server: the resident batch server (B > 1; bserve_eligible: a one-wave
// deterministic XYD batch) or the lone-grid server.
template <typename T>
int launch_serve_t(mgdp_vi *vi, unsigned int served) {
    const ViPlan &p = vi->plan;
    const bool batch = vi->d.B > 1;
    MGDP_CHECK(!batch || vi->k.bserve, MGDP_E_INVALID, "batch server: not a one-wave deterministic XYD batch");
    const Geo g = make_geo(vi);
    TimedPair tp;
    if (int rc = timed_begin(vi, -1, &tp)) return rc;
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
    if (int rc = timed_begin(vi, k, &tp)) return rc;
    if constexpr (MAP == MGDP_MAP_CELL) {
        if (vi->plan.sweep_pipe == 1) return launch_sweep_pipe<T, MODEL, SLIP, 1>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 2) return launch_sweep_pipe<T, MODEL, SLIP, 2>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 3) return launch_sweep_pipe<T, MODEL, SLIP, 3>(vi, Vin, Vout, k, check_prev, tp);
        if (vi->plan.sweep_pipe == 4) return launch_sweep_pipe<T, MODEL, SLIP, 4>(vi, Vin, Vout, k, check_prev, tp);
    }
    return launch_sweep_kernel<T, MODEL, SLIP, MAP, false>(vi, Vin, Vout, k, check_prev, tp);
}

// Dispatch on (dtype, model, slip, mapping).
template <template <typename, int, bool, int> class F, typename... Args>
int dispatch(mgdp_vi *vi, Args... args) {
    const bool slip = vi->d.slip_p >= 0.0;
    const bool sa = vi->d.mapping == MGDP_MAP_SA;
    if (vi->d.dtype == MGDP_F32) {
        if (vi->d.model == MGDP_MODEL_XYD) {
            if (slip) return sa ? F<float, 0, true, 1>::run(vi, args...) : F<float, 0, true, 0>::run(vi, args...);
            return sa ? F<float, 0, false, 1>::run(vi, args...) : F<float, 0, false, 0>::run(vi, args...);
        }
        return sa ? F<float, 1, false, 1>::run(vi, args...) : F<float, 1, false, 0>::run(vi, args...);
    }
    if (vi->d.model == MGDP_MODEL_XYD) {
        if (slip) return sa ? F<double, 0, true, 1>::run(vi, args...) : F<double, 0, true, 0>::run(vi, args...);
        return sa ? F<double, 0, false, 1>::run(vi, args...) : F<double, 0, false, 0>::run(vi, args...);
    }
    return sa ? F<double, 1, false, 1>::run(vi, args...) : F<double, 1, false, 0>::run(vi, args...);
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

// Read the reduction the last fused launch published to host-mapped memory: max k, max dV, min k.
int reduce_env(mgdp_vi *vi, int32_t *kmax, double *dvmax) {
    // The last workgroup (or the reduce kernel) publishes {kmax, dV hi, dV lo, kmin} to host-mapped
    // memory as four epoch-tagged words; the persistent server publishes three (words 5..7).  Poll them rather
    // than synchronise the stream (lower completion latency); everything else stays stream-ordered.
    // Poll the stream now and then to surface faults -- and, in serving mode, to relaunch a server
    // that left before it saw the request.
    const volatile unsigned long long *h = vi->h_out;
    const unsigned long long ep = (unsigned long long)vi->epoch;
    const bool served = vi->serving;                 // a resident server answers (a relaunch may be needed)
    const bool tagged = served && vi->d.B == 1;      // ... in the lone server's words [5..7]
    auto ready = [&]() -> bool {
        if (!tagged) return (h[0] >> 32) == ep && (h[1] >> 32) == ep && (h[2] >> 32) == ep && (h[3] >> 32) == ep;
        return (h[5] >> 32) == ep && (h[6] >> 32) == ep && (h[7] >> 32) == ep;
    };
    int relaunches = 0;
    // probe knobs (MGDP_QUERY_SPINS, MGDP_QUERY_AFTER_US, MGDP_SPIN_PAUSE): how often the wait
    // queries the stream, after how long, and whether each spin pauses
    static const int q_mask = [] { const char *e = std::getenv("MGDP_QUERY_SPINS"); return e ? std::atoi(e) - 1 : 1023; }();
    static const double q_after = [] { const char *e = std::getenv("MGDP_QUERY_AFTER_US"); return e ? std::atof(e) : 0.0; }();
    static const bool s_pause = [] { const char *e = std::getenv("MGDP_SPIN_PAUSE"); return e && std::atoi(e) != 0; }();
    bool query = q_after <= 0.0;
    const auto t_wait = std::chrono::steady_clock::now();
    for (uint64_t spin = 0; !ready(); ++spin) {
        if (s_pause) __builtin_ia32_pause();
        if ((spin & (uint64_t)q_mask) == (uint64_t)q_mask) {
            if (!query) {
                query = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_wait).count() > q_after;
                if (!query) continue;
            }
            const hipError_t q = hipStreamQuery(vi->stream);
            if (q == hipSuccess) {
                if (ready()) break;
                if (served && relaunches < 4) {
                    ++relaunches;
                    DeviceGuard guard(vi->d.device);  // the served fast path of mgdp_vi_solve holds none
                    if (int rc = launch_serve(vi, vi->epoch - 1u)) return rc;
                    continue;
                }
                MGDP_CHECK(false, MGDP_E_HIP, "fused launch finished without publishing its result (epoch %u)", vi->epoch);
            }
            if (q != hipErrorNotReady) return hip_fail(q, "fused value-iteration launch", __FILE__, __LINE__);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
#ifdef MGDP_SERVE_TRACE
    // trace build (tools/probe_serve_trace.sh): server-side s_memrealtime stamps, 10 ns ticks --
    // [8] request seen by the workgroup, [9] result about to be published
    // The server stores its stamps behind the result (so the publish is the plain build's), word 9 last:
    // wait for it to change (bounded: a relaunched server's first solve may repeat nothing).
    if (tagged) {
        static unsigned long long last9 = 0;
        for (int spin = 0; spin < 100000 && h[9] == last9; ++spin) __builtin_ia32_pause();
        last9 = h[9];
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (tagged) {  // each block of 1000 solves: mean GPU-side time, the shader clock over it, and when
        static double n = 0, solve = 0, cyc = 0;
        static const auto t_first = std::chrono::steady_clock::now();
        n += 1;
        solve += (double)(h[9] - h[8]) * 0.01;
        cyc += (double)(h[15] - h[14]);
        // the pair loop's shader-clock stamps (fused_serve_pair, words 18..23; all 0 on other loops):
        // seen -> first pair, one steady pair split at reads landed / last VALU / barrier passed, the
        // whole loop, loop left -> publish
        static double seg[7] = {0, 0, 0, 0, 0, 0, 0};
        const volatile unsigned long long *s = h + 18;
        if (s[0] && s[5]) {
            seg[0] += (double)(s[0] - h[14]);
            if (s[1] && s[4]) {
                seg[1] += (double)(s[2] - s[1]);
                seg[2] += (double)(s[3] - s[2]);
                seg[3] += (double)(s[4] - s[3]);
                seg[4] += (double)(s[4] - s[1]);
            }
            seg[5] += (double)(s[5] - s[0]);
            seg[6] += (double)(h[15] - s[5]);
        }
        // the depth form (vi_serve_depth.h) stamps s[0] search start and s[5] search end (the columns "seen->first
        // pair", "loop" and "left->publish" then read seen -> search start, search, search end -> publish) and,
        // behind the publish, word 10: its V and pi stores issued.  That word is the previous solve's by now.
        static double stored = 0;
        static unsigned long long prev15 = 0;
        if (prev15 && h[10] > prev15 && h[10] < h[14]) stored += (double)(h[10] - prev15);
        prev15 = h[15];
        if ((long long)n % 1000 == 0) {
            std::fprintf(stderr, "serve trace depth: cycles per solve: publish -> V and pi stores issued %.1f\n", stored / 1000.0);
            stored = 0;
        }
        if ((long long)n % 1000 == 0) {
            std::fprintf(stderr, "serve trace pair: cycles per solve: seen->first pair %.1f, steady pair %.1f = reads %.1f + valu %.1f + "
                                 "flags/barrier %.1f, loop %.1f, left->publish %.1f, seen->publish %.1f\n",
                         seg[0] / 1000.0, seg[4] / 1000.0, seg[1] / 1000.0, seg[2] / 1000.0, seg[3] / 1000.0, seg[5] / 1000.0,
                         seg[6] / 1000.0, cyc / 1000.0);
            for (double &x : seg) x = 0;
            const double t_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_first).count();
            std::fprintf(stderr, "serve trace: solves %.0f-%.0f, t %.1f ms, request seen -> publish %.3f us, sclk %.0f MHz (sweeps %llu)\n",
                         n - 999, n, t_ms, solve / 1000.0, cyc / solve, (unsigned long long)(h[5] & 0xffffffffull));
            solve = 0;
            cyc = 0;
        }
    }
#endif
    unsigned long long km, dvb, kmin;
    if (tagged) {
        km = kmin = h[5] & 0xffffffffull;
        dvb = ((h[6] & 0xffffffffull) << 32) | (h[7] & 0xffffffffull);
    } else {
        km = h[0] & 0xffffffffull;
        dvb = ((h[1] & 0xffffffffull) << 32) | (h[2] & 0xffffffffull);
        kmin = h[3] & 0xffffffffull;
    }
    std::memcpy(&vi->dv_red, (const void *)&dvb, sizeof(double));  // non-negative doubles order like their bits
    vi->k_min = (int)kmin;
    vi->k_max = (int)km;
    vi->k_done_valid = true;
    if (kmax) *kmax = (int32_t)km;
    if (dvmax) *dvmax = vi->dv_red;
    return 0;
}

// Persistent solver hand-off (lone grid on the one-thread-per-cell fused path; the shape is the plan's).
bool serve_eligible(const mgdp_vi *vi) { return vi->kn.persistent && vi->plan.serve_shape; }
// The resident batch server (vi_bserve_kernel): a deterministic XYD batch on one wave per grid
// (the wave2 kernel with its in-launch reduction) that fits the server's resident capacity, solved
// with launch timing off (a timed solve is a launch, so kernel_time() keeps timing one solve per
// launch), from V_0 = 0 under the own rule with at least one sweep.  Its buffers exist only where
// the plan wants a batch server and it has a resident capacity.
bool bserve_eligible(const mgdp_vi *vi) {
    return vi->kn.persistent && vi->d_breq && vi->d_gk && !vi->timing && vi->d.B > 1 &&
           (vi->d.B <= vi->plan.bserve_cap || vi->plan.bserve_any) &&
           !vi->plan.opts && vi->d.method == MGDP_METHOD_FUSED && vi->d.horizon == 0 && vi->d.max_sweeps >= 1;
}
bool served_eligible(const mgdp_vi *vi) { return serve_eligible(vi) || bserve_eligible(vi); }
// Ask a resident server to leave and drain the stream.  Every entry point that enqueues other
// work on the stream, or reads results, calls this first.  A grid handed over for the next request
// but not yet served goes to d_cells here, so every other launch sees it.
// drain = false (mgdp_vi_synchronize): wait for the server's exit word -- its V / pi stores are
// then complete and visible, and nothing else is queued behind it -- instead of the stream's
// completion signal, which a later device synchronize still observes.
// Wait for the exit word of the latest server launch (its own tag: a late store of an earlier
// server cannot satisfy it); a server that never started or faulted is reported by the stream.
// Add a departed server's clock words (written before its exit word, which is a release) once.
void account_server_clock(mgdp_vi *vi) {
    const volatile unsigned long long *h = vi->h_out;
    if (vi->serve_tag == 0 || vi->clk_tag == vi->serve_tag || h[11] != vi->serve_tag) return;
    std::atomic_thread_fence(std::memory_order_acquire);
    vi->clk_cycles += (double)h[kHoutClk];
    vi->clk_ticks += (double)h[kHoutClk + 1];
    vi->clk_busy += (double)h[kHoutClk + 2];
    vi->clk_solves += (double)h[kHoutClk + 3];
    // the departed launch's requests by path (Loop::serve_pair writes them; other servers leave them 0)
    for (int i = 0; i < 3; ++i) {
        vi->path_counts[i] += (long long)h[kHoutPath + 1 + i];
        vi->h_out[kHoutPath + 1 + i] = 0;
    }
    ++vi->clk_launches;
    vi->clk_tag = vi->serve_tag;
}
int wait_server_exit(mgdp_vi *vi) {
    const volatile unsigned long long *h = vi->h_out;
    for (uint64_t spin = 0; h[11] != vi->serve_tag; ++spin) {
        if ((spin & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(vi->stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return hip_fail(q, "persistent server", __FILE__, __LINE__);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    account_server_clock(vi);
    return 0;
}
int server_stop(mgdp_vi *vi, bool drain = true) {
    if (vi->serving) {
        __atomic_store_n(vi->h_out + kHoutReq, kServeQuit, __ATOMIC_RELEASE);
        vi->serving = false;
        if (drain) {
            MGDP_HIP(hipStreamSynchronize(vi->stream));
            account_server_clock(vi);
        } else if (int rc = wait_server_exit(vi)) {
            return rc;
        }
    }
    // Whatever the caller enqueues next follows the departed server on the stream, so its exit
    // word no longer says the stream is idle (mgdp_vi_synchronize's shortcut).
    vi->exiting = false;
    if (vi->pending_src) {
        MGDP_HIP(hipMemcpyAsync(vi->d_cells, reinterpret_cast<const void *>(vi->pending_src), vi->HW, hipMemcpyDefault,
                                vi->stream));
        MGDP_HIP(hipStreamSynchronize(vi->stream));
        vi->pending_src = 0;
    }
    return 0;
}
// Post the next request word: epoch, plus kServeNewCells and the tagged source word when a new
// grid is pending (source first, then the request, both release stores: x86 keeps them in order).
void post_request(mgdp_vi *vi) {
    if (++vi->epoch == 0u) ++vi->epoch;  // never 0: a batch server publishes tagged with it (publish())
    unsigned long long w = (unsigned long long)vi->epoch;
    if (vi->last_req) w |= kServeLast;
    if (vi->pending_src) {
        __atomic_store_n(vi->h_out + kHoutReq + 1, vi->pending_src | ((w & 0xffffull) << 48), __ATOMIC_RELEASE);
        w |= kServeNewCells;
        vi->pending_src = 0;
    }
    __atomic_store_n(vi->h_out + kHoutReq, w, __ATOMIC_RELEASE);
}
// Hand a new lone grid to a resident server (no drain): true if it was taken.
bool serve_handoff(mgdp_vi *vi, const void *src) {
    const unsigned long long a = (unsigned long long)(uintptr_t)src;
    if (!vi->serving || !serve_eligible(vi) || (a >> 48) != 0) return false;
    vi->pending_src = a;
    return true;
}
// Post request `epoch` (the server serves any request word != the last epoch it served) and make
// sure a server is resident; reduce_env then waits for the published result.
int serve_request(mgdp_vi *vi) {
    // A server idle for more than half its limit may be leaving: restart it deterministically
    // (quit + drain, then a fresh launch) instead of discovering its exit while polling.
    if (vi->serving) {
        const double idle_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - vi->serve_last).count();
        if (idle_us * 100.0 > 0.5 * (double)vi->serve_idle_ticks)
            if (int rc = server_stop(vi)) return rc;
    }
    post_request(vi);
    if (!vi->serving) {
        // A server that left after its last request (mgdp_vi_solve_last) may still be storing V / pi and its
        // exit words: the new launch queues behind it on the stream in any case, and its clock and path words
        // are counted only once its exit word is seen (a depth-form solve publishes well ahead of them).
        if (vi->exiting)
            if (int rc = wait_server_exit(vi)) return rc;
        vi->exiting = false;  // a departing earlier server is no longer the stream's last work
        if (int rc = launch_serve(vi, vi->epoch - 1u)) return rc;
        vi->serving = true;
    }
    vi->fresh = 0;
    return 0;
}

double shard_max(const unsigned long long *sh) {
    double m = 0.0;
    for (int i = 0; i < 8; ++i) {
        double v;
        std::memcpy(&v, &sh[i], sizeof(double));
        m = v > m ? v : m;
    }
    return m;
}

// Sweep method: run sweeps k_done+1.. with the device-global rule; force = run exactly to k_stop.
int sweep_run(mgdp_vi *vi, int k_stop, bool force, double *dv_out) {
    const int chunk = 8;
    std::vector<unsigned long long> host(8 * chunk);
    double dv = 0.0;
    while (vi->k_done < k_stop) {
        const size_t ev0 = vi->ev_sweep.size();
        const int n = std::min(chunk, k_stop - vi->k_done);
        for (int i = 1; i <= n; ++i)
            if (int rc = dispatch<SweepF>(vi, vi->k_done + i, force ? 0 : 1, false)) return rc;
        MGDP_HIP(hipMemcpyAsync(host.data(), vi->d_shards + (long long)vi->k_done * 8, 8 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, vi->stream));
        MGDP_HIP(hipStreamSynchronize(vi->stream));
        int last = vi->k_done + n;
        bool stop = false;
        for (int i = 0; i < n; ++i) {
            dv = shard_max(&host[8 * i]);
            if (!force && dv < vi->d.tol) {
                last = vi->k_done + i + 1;
                stop = true;
                break;
            }
        }
        for (size_t i = ev0; i < vi->ev_sweep.size(); ++i)
            if (vi->ev_sweep[i] > last) vi->ev_sweep[i] = INT32_MAX;
        vi->k_done = last;
        vi->cur = last & 1;
        if (stop) break;
    }
    if (dv_out) *dv_out = dv;
    return 0;
}

int validate_cells(const mgdp_vi_desc &d, const uint8_t *cells) {
    const int HW = d.W * d.H;
    for (int b = 0; b < d.B; ++b) {
        const uint8_t *c = cells + (int64_t)b * HW;
        int doors = 0, keys = 0;
        for (int y = 0; y < d.H; ++y)
            for (int x = 0; x < d.W; ++x) {
                const int t = c[y * d.W + x];
                const bool border = x == 0 || y == 0 || x == d.W - 1 || y == d.H - 1;
                bool ok = t == T_EMPTY || t == T_WALL || t == T_FLOOR || t == T_GOAL || t == T_LAVA;
                if (d.model == MGDP_MODEL_DOORKEY) {
                    if (t == T_DOOR) { ++doors; ok = !border; }
                    if (t == T_KEY) { ++keys; ok = !border; }
                }
                MGDP_CHECK(ok, MGDP_E_UNSUPPORTED, "grid %d cell (%d,%d): type %d is outside the %s model", b, x, y, t,
                           d.model == MGDP_MODEL_XYD ? "XYD" : "DoorKey");
                MGDP_CHECK(!(border && (t == T_EMPTY || t == T_FLOOR || (d.lava_mode == MGDP_LAVA_NODEATH && t == T_LAVA))),
                           MGDP_E_UNSUPPORTED,
                           "grid %d border cell (%d,%d) is walkable; the model needs a closed border", b, x, y);
            }
        if (d.model == MGDP_MODEL_DOORKEY)
            MGDP_CHECK(doors == 1 && keys == 1, MGDP_E_UNSUPPORTED,
                       "grid %d: DoorKey model needs exactly one door and one key (found %d, %d)", b, doors, keys);
    }
    return 0;
}

}  // namespace

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
    for (auto &p : vi->ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &p : vi->ev_pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    (void)hipFree(vi->d_cells);
    (void)hipFree(vi->d_V[0]);
    (void)hipFree(vi->d_V[1]);
    (void)hipFree(vi->d_pi);
    (void)hipFree(vi->d_kenv);
    (void)hipFree(vi->d_kexec);
    (void)hipFree(vi->d_order);
    (void)hipFree(vi->d_dvenv);
    (void)hipFree(vi->d_shards);
    (void)hipFree(vi->d_red);
    (void)hipFree(vi->d_pub1);
    (void)hipFree(vi->d_gk);
    (void)hipFree(vi->d_breq);
    (void)hipFree(vi->d_rgoal);
    (void)hipFree(vi->d_pi_t);
    (void)hipFree(vi->d_eval);
    (void)hipFree(vi->d_pi_stage);
    (void)hipFree(vi->d_vt_stage);
    (void)hipFree(vi->d_occ_err);
    (void)hipFree(vi->d_occ_tab);
    for (void *p : vi->d_occ_stage) (void)hipFree(p);
    if (vi->h_out) (void)hipHostFree(vi->h_out);
    if (vi->h_stage) (void)hipHostFree(vi->h_stage);
    if (vi->own_stream) (void)hipStreamDestroy(vi->stream);
    delete vi;
    return 0;
}

int mgdp_vi_set_stream(mgdp_vi *vi, void *s) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    if (vi->own_stream) { (void)hipStreamDestroy(vi->stream); vi->own_stream = false; vi->stream = nullptr; }
    if (s) {
        vi->stream = (hipStream_t)s;
    } else {
        MGDP_HIP(hipStreamCreateWithFlags(&vi->stream, hipStreamNonBlocking));
        vi->own_stream = true;
    }
    return 0;
}

namespace {
int cells_dispatch(mgdp_vi *vi);  // the dispatch order from the cells just loaded (below)
}  // namespace

int mgdp_vi_load_cells(mgdp_vi *vi, const uint8_t *cells) {
    MGDP_CHECK(vi && cells, MGDP_E_INVALID, "null argument");
    if (int rc = validate_cells(vi->d, cells)) return rc;
    // a resident lone-grid server takes the grid with its next request: staged in host memory
    // (a solve is synchronous, so the server is not reading the staging buffer now)
    if (vi->h_stage && vi->serving && serve_eligible(vi)) {
        std::memcpy(vi->h_stage, cells, vi->HW);
        if (serve_handoff(vi, vi->d_stage)) {
            vi->cells_loaded = true;
            vi->k_done_valid = false;
            return 0;
        }
    }
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    std::vector<uint8_t> pad((size_t)vi->d.B * vi->HWp, 0);
    for (int b = 0; b < vi->d.B; ++b) std::memcpy(&pad[(size_t)b * vi->HWp], cells + (size_t)b * vi->HW, vi->HW);
    MGDP_HIP(hipMemcpyAsync(vi->d_cells, pad.data(), pad.size(), hipMemcpyHostToDevice, vi->stream));
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    vi->cells_loaded = true;
    vi->k_done_valid = false;
    vi->order_valid = false;
    vi->solves_since_load = 0;
    return cells_dispatch(vi);
}

int mgdp_vi_load_cells_device(mgdp_vi *vi, const uint8_t *d_cells) {
    MGDP_CHECK(vi && d_cells, MGDP_E_INVALID, "null argument");
    // The resident server reads the bytes itself with its next request, unordered with respect to
    // any stream: only on the handle's own stream, where no caller kernel can still be producing
    // them.  On a caller-bound stream (mgdp_vi_set_stream) the copy below is ordered after whatever
    // the caller enqueued there before this call.
    if (vi->own_stream && serve_handoff(vi, d_cells)) {
        vi->cells_loaded = true;
        vi->k_done_valid = false;
        return 0;
    }
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipMemcpy2DAsync(vi->d_cells, vi->HWp, d_cells, vi->HW, vi->HW, vi->d.B, hipMemcpyDeviceToDevice, vi->stream));
    vi->cells_loaded = true;
    vi->k_done_valid = false;
    vi->order_valid = false;
    vi->solves_since_load = 0;
    return cells_dispatch(vi);
}

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
}  // namespace

int mgdp_vi_reset(mgdp_vi *vi) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (!vi->order_valid && vi->kn.order_src == 2 && vi->solves_since_load > 0 && order_eligible(vi)) {
        if (int rc = server_stop(vi)) return rc;
        if (int rc = learn_dispatch(vi)) return rc;
    }
    if (vi->d.method == MGDP_METHOD_SWEEP) {  // V_0 = 0 and an empty dV trace
        const size_t BS = (size_t)vi->d.B * vi->S;
        MGDP_HIP(hipMemsetAsync(vi->d_V[0], 0, BS * vi->tsize, vi->stream));
        MGDP_HIP(hipMemsetAsync(vi->d_shards, 0, sizeof(unsigned long long) * 8 * (size_t)(vi->d.max_sweeps + 1), vi->stream));
    }
    vi->fresh = 1;  // the next fused launch ignores kenv/dvenv and starts from V_0 = 0
    vi->cur = 0;
    vi->k_done = 0;
    vi->k_min = 0;
    vi->k_done_valid = false;
    vi->sweeps = 0;
    vi->converged = 0;
    vi->evaluated = false;
    return 0;
}

int mgdp_vi_run_local(mgdp_vi *vi, int32_t *k_local_max) {
    MGDP_CHECK(vi && k_local_max, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->cells_loaded, MGDP_E_INVALID, "no cells loaded");
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
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
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
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
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts, MGDP_E_UNSUPPORTED,
               "the device protocol runs the fused method without horizon / lava options");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    vi->k_done_valid = false;
    return launch_fused(vi, -1, reinterpret_cast<unsigned long long *>(d_pub), (const long long *)nullptr);
}

int mgdp_vi_run_to_dev(mgdp_vi *vi, const int64_t *d_k, int64_t *d_pub) {
    MGDP_CHECK(vi && d_k && d_pub, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts, MGDP_E_UNSUPPORTED,
               "the device protocol runs the fused method without horizon / lava options");
    MGDP_CHECK(!vi->fresh, MGDP_E_INVALID, "mgdp_vi_run_to_dev before mgdp_vi_run_local_dev");
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
    DeviceGuard guard(vi->d.device);
    vi->k_done_valid = false;
    return launch_fused(vi, 0, reinterpret_cast<unsigned long long *>(d_pub), reinterpret_cast<const long long *>(d_k));
}

int mgdp_vi_run_to_dev_sync(mgdp_vi *vi, const int64_t *d_kdv, int32_t *k_out, double *dv_out, double *dv_rule_out) {
    MGDP_CHECK(vi && d_kdv, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts, MGDP_E_UNSUPPORTED,
               "the device protocol runs the fused method without horizon / lava options");
    MGDP_CHECK(!vi->fresh, MGDP_E_INVALID, "mgdp_vi_run_to_dev_sync before mgdp_vi_run_local_dev");
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
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
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
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

int mgdp_vi_solve(mgdp_vi *vi, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    // Resident lone-grid server: a solve is a request word and a wait on host memory, so the
    // steady state makes no HIP call at all (no device guard either); anything else -- a server
    // that may be leaving, a rounding-level fallback sweep -- takes the general path below.
    // (a batch whose learned dispatch order is due takes the general path: mgdp_vi_reset learns it)
    const bool learn_due = vi->d.B > 1 && !vi->order_valid && vi->kn.order_src == 2 && vi->solves_since_load > 0;
    if (vi->serving && served_eligible(vi) && vi->d.horizon == 0 && !learn_due) {
        const double idle_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - vi->serve_last).count();
        if (idle_us * 100.0 <= 0.5 * (double)vi->serve_idle_ticks) {
            vi->cur = 0;
            vi->k_done = 0;
            vi->k_done_valid = false;
            post_request(vi);
            vi->fresh = 0;
            int32_t k = 0;
            if (int rc = reduce_env(vi, &k, nullptr)) return rc;
            vi->serve_last = std::chrono::steady_clock::now();
            const double dv = vi->dv_red;
            // a batch is complete at K when every grid ended there or at an exact fixed point (mgdp_vi_run_to)
            const bool at_k = vi->d.B == 1 || vi->k_min == k || (vi->dv_red == 0.0 && vi->k_min > 0);
            if (vi->d.B > 1) ++vi->solves_since_load;
            if (at_k && (dv < vi->d.tol || k >= vi->d.max_sweeps)) {
                vi->k_done = k;
                vi->sweeps = k;
                vi->converged = dv < vi->d.tol;
                if (sweeps_out) *sweeps_out = k;
                if (dv_out) *dv_out = dv;
                if (converged_out) *converged_out = vi->converged;
                return 0;
            }
            // rounding broke the contraction: continue under the global rule on the general path
            double dv2 = dv;
            if (int rc = mgdp_vi_run_to(vi, k, &dv2)) return rc;
            while (!(dv2 < vi->d.tol) && k < vi->d.max_sweeps) {
                if (int rc = mgdp_vi_sweep(vi, &dv2)) return rc;
                ++k;
            }
            if (int rc = mgdp_vi_finish(vi, k)) return rc;
            vi->converged = dv2 < vi->d.tol;
            if (sweeps_out) *sweeps_out = k;
            if (dv_out) *dv_out = dv2;
            if (converged_out) *converged_out = vi->converged;
            return 0;
        }
    }
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
    while (vi->d.horizon == 0 && !(dv < vi->d.tol) && k < vi->d.max_sweeps) {  // contraction broken by rounding: global rule
        if (int rc = mgdp_vi_sweep(vi, &dv)) return rc;
        ++k;
    }
    if (int rc = mgdp_vi_finish(vi, k)) return rc;
    ++vi->solves_since_load;
    vi->converged = vi->d.horizon > 0 ? 1 : dv < vi->d.tol;  // a finite horizon is exact after H sweeps
    if (sweeps_out) *sweeps_out = k;
    if (dv_out) *dv_out = dv;
    if (converged_out) *converged_out = vi->converged;
    return 0;
}

// The sharded solve with the library's own collectives (include/mgdp.h, ABI 11): the device
// protocol of distributed.py with RCCL called from here on the handle's stream instead of through
// torch.distributed -- run_local_dev publishes {K_r, E_r bits, kmin, 0} into the communicator's
// device words, ncclAllReduce(MAX) of the first two is enqueued right behind it, the gate (or
// run_to(K)) reads them on the device, and the host waits once on host-mapped words.  Only when
// some grid anywhere stopped its own rule with dV > 0 (E != 0: slip, rounding, a cap) is dV(K)
// all-reduced too, and only a rounding-level breach of the contraction runs fallback sweeps.
namespace {
int comm_max_double(mgdp_comm *c, hipStream_t s, double *x) {
    // one word through the communicator's device buffer: non-negative doubles order like their bits
    int64_t *h = comm_host_word(c), *d = comm_proto(c) + 5;
    std::memcpy(h, x, sizeof(double));
    MGDP_HIP(hipMemcpyAsync(d, h, sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (int rc = comm_allreduce_max_dev(c, d, 1, s)) return rc;
    MGDP_HIP(hipMemcpyAsync(h, d, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    MGDP_HIP(hipStreamSynchronize(s));
    comm_note_host_wait(c);
    std::memcpy(x, h, sizeof(double));
    return 0;
}
}  // namespace

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
    while (!(dv < vi->d.tol) && k < vi->d.max_sweeps) {  // contraction broken by rounding: global rule
        if (int rc = mgdp_vi_sweep(vi, &dv)) return rc;
        if (int rc = comm_max_double(comm, vi->stream, &dv)) return rc;
        ++k;
        vi->dv_red = dv;
    }
    if (int rc = mgdp_vi_finish(vi, k)) return rc;
    ++vi->solves_since_load;
    vi->converged = dv < vi->d.tol;
    if (sweeps_out) *sweeps_out = k;
    if (dv_out) *dv_out = dv;
    if (converged_out) *converged_out = vi->converged;
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
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && vi->d.horizon == 0, MGDP_E_INVALID,
               "resume: the fused method with an infinite horizon");
    MGDP_CHECK(k >= 1 && k < vi->d.max_sweeps, MGDP_E_INVALID, "resume: sweep %d outside [1, max_sweeps)", k);
    MGDP_CHECK(!(dv < vi->d.tol), MGDP_E_INVALID,
               "resume: the checkpoint has converged (dV %g < tol %g); its V and pi are final", dv, vi->d.tol);
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    // the copies below go through the null stream: drain the handle's own (or a caller-bound,
    // possibly non-blocking) stream first, so no earlier launch still reads V / kenv / dvenv
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    const size_t BS = (size_t)vi->d.B * vi->S;
    MGDP_HIP(hipMemcpy(vi->d_V[0], V, BS * vi->tsize, hipMemcpyHostToDevice));
    std::vector<int32_t> kk((size_t)vi->d.B, k);
    std::vector<double> dd((size_t)vi->d.B, dv);
    MGDP_HIP(hipMemcpy(vi->d_kenv, kk.data(), kk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MGDP_HIP(hipMemcpy(vi->d_kexec, kk.data(), kk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MGDP_HIP(hipMemcpy(vi->d_dvenv, dd.data(), dd.size() * sizeof(double), hipMemcpyHostToDevice));
    vi->fresh = 0;  // the next fused launch continues each grid from kenv / dvenv and V in HBM
    vi->cur = 0;
    vi->k_done = k;
    vi->k_min = k;
    vi->k_done_valid = false;
    vi->sweeps = k;
    vi->converged = 0;
    int32_t K = k;
    double dv2 = dv;
    if (int rc = mgdp_vi_run_local(vi, &K)) return rc;
    if (int rc = mgdp_vi_run_to(vi, K, &dv2)) return rc;
    while (!(dv2 < vi->d.tol) && K < vi->d.max_sweeps) {  // contraction broken by rounding: global rule
        if (int rc = mgdp_vi_sweep(vi, &dv2)) return rc;
        ++K;
    }
    if (int rc = mgdp_vi_finish(vi, K)) return rc;
    vi->converged = dv2 < vi->d.tol;
    if (sweeps_out) *sweeps_out = K;
    if (dv_out) *dv_out = dv2;
    if (converged_out) *converged_out = vi->converged;
    return 0;
}

// Policy evaluation, improvement and policy iteration (DESIGN.md sections 13 and 19; kernels in vi_eval.h and
// vi_eval_opts.h).  One implementation per operation, over (pi, T rows, V_t): the plain ABI names are its
// strict form (no option handle, T = 1, no V_t), the *_opts names check T / V_t and take any handle.
// An evaluation is the solve's protocol on vi_eval_kernel: every grid to its own stop, the grids that
// stopped with dV != 0 to K = max k_e, then the global rule sweep by sweep if dV(K) >= tol; on a finite
// horizon it is one launch of exactly H sweeps.
extern "C++" {  // the launch helpers are templates
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

// The launch of an evaluation kernel (vi_eval_kernel, vi_eval_nd_kernel, vi_eval_fh_kernel): the arguments
// the three share, the kernel's own (`tail`), then in_kernel_reduce and the epoch.
template <typename T, typename K, typename... Tail>
int launch_eval_kernel(mgdp_vi *vi, K kern, const int8_t *pi_src, Tail... tail) {
    const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
    if (s.lds > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, s.lds));
    TimedPair tp;
    if (int rc = timed_begin(vi, -1, &tp)) return rc;
    hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(s.block), s.lds, vi->stream, tp.a, tp.b, 0, eval_geo(vi, s),
                          make_coef<T>(vi), vi->d_cells, (T *)vi->d_V[0], pi_src, vi->d_pi, vi->d_kenv, vi->d_dvenv,
                          vi->d_red, vi->d_ticket, vi->d_hout, vi->d_eval, tail...,
                          vi->d.B <= vi->kn.inkernel_max ? 1 : 0, next_host_epoch(vi));
    MGDP_HIP(hipGetLastError());
    vi->fresh = 0;
    if (vi->d.B > vi->kn.inkernel_max) {
        launch_reduce(vi, vi->d_hout);
        MGDP_HIP(hipGetLastError());
    }
    return 0;
}

// Dispatch on (dtype, model, slip, NoDeath lava); the mapping does not apply (one thread per cell).  DoorKey
// has neither slip nor NoDeath (mgdp_vi_create), so neither is instantiated.
template <typename T, template <typename, int, bool, bool> class F, typename... Args>
int dispatch_eval_t(mgdp_vi *vi, Args... args) {
    if (vi->d.model == MGDP_MODEL_DOORKEY) return F<T, MGDP_MODEL_DOORKEY, false, false>::run(vi, args...);
    const bool nd = vi->d.lava_mode == MGDP_LAVA_NODEATH;
    if (vi->d.slip_p >= 0.0) return nd ? F<T, MGDP_MODEL_XYD, true, true>::run(vi, args...) : F<T, MGDP_MODEL_XYD, true, false>::run(vi, args...);
    return nd ? F<T, MGDP_MODEL_XYD, false, true>::run(vi, args...) : F<T, MGDP_MODEL_XYD, false, false>::run(vi, args...);
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
    template <bool TI, bool VT>
    static int launch(mgdp_vi *vi, const int8_t *pi_src, void *d_vt) {
        return launch_eval_kernel<T>(vi, vi_eval_fh_kernel<T, MODEL, SLIP, ND, TI, VT>, pi_src, (const T *)vi->d_rgoal,
                                     (T *)d_vt, vi->d.horizon);
    }
    static int run(mgdp_vi *vi, const int8_t *pi_src, bool ti, void *d_vt) {
        const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
        constexpr int max_block = kEvalFhBlock<T, MODEL>;
        MGDP_CHECK(s.block <= max_block, MGDP_E_UNSUPPORTED, "policy evaluation: %d cell slots exceed the kernel's %d threads",
                   s.block, max_block);
        if (ti) return d_vt ? launch<true, true>(vi, pi_src, d_vt) : launch<true, false>(vi, pi_src, d_vt);
        return d_vt ? launch<false, true>(vi, pi_src, d_vt) : launch<false, false>(vi, pi_src, d_vt);
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
    if (!vi->order_valid && vi->kn.order_src == 2 && vi->solves_since_load > 0 && order_eligible(vi))
        if (int rc = learn_dispatch(vi)) return rc;
    if (int rc = eval_buffers(vi)) return rc;
    MGDP_HIP(hipMemsetAsync(vi->d_eval, 0xff, sizeof(unsigned long long), vi->stream));
    vi->fresh = 1;
    vi->cur = 0;
    vi->k_done = vi->k_min = 0;
    vi->k_done_valid = false;
    vi->sweeps = vi->converged = 0;
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
int eval_finish(mgdp_vi *vi, int32_t k, double dv, int32_t converged, int32_t *sweeps_out, double *dv_out,
                int32_t *converged_out) {
    vi->k_done = k;
    vi->k_done_valid = false;  // the protocol entry points need a reset after an evaluation
    vi->sweeps = k;
    vi->converged = converged;
    if (sweeps_out) *sweeps_out = k;
    if (dv_out) *dv_out = dv;
    if (converged_out) *converged_out = converged;
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
    while (!(dv < vi->d.tol) && k < vi->d.max_sweeps) {  // contraction broken by rounding: global rule
        if (int rc = dispatch_eval<EvalF>(vi, k + 1, nullptr)) return rc;
        if (int rc = reduce_env(vi, &km, &dv)) return rc;
        ++k;
    }
    return eval_finish(vi, k, dv, dv < vi->d.tol, sweeps_out, dv_out, converged_out);
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
    return eval_finish(vi, k, dv, 1, sweeps_out, dv_out, converged_out);  // a finite horizon is exact after H sweeps
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

// ---- the forward pass of a policy (vi_occupancy.h) ----
// It reads the handle's cells and options only: V, pi, kenv and the protocol state stay as they are.
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
struct OccupancyF {
    template <bool TI, bool MT>
    static int launch(mgdp_vi *vi, const int8_t *d_pi, const int32_t *d_start, const void *d_mu0, int N, void *d_mu,
                      void *d_occ, void *d_ret, void *d_mu_t) {
        const EvalShape s = eval_shape(vi->HW, vi->HWp, vi->S, vi->tsize);
        auto kern = vi_occupancy_kernel<T, SLIP, ND, TI, MT>;
        if (s.lds > 64 * 1024) MGDP_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, s.lds));
        TimedPair tp;
        if (int rc = timed_begin(vi, -1, &tp)) return rc;
        hipExtLaunchKernelGGL(kern, dim3(vi->d.B), dim3(s.block), s.lds, vi->stream, tp.a, tp.b, 0, eval_geo(vi, s),
                              make_coef<T>(vi), vi->d_cells, d_pi, d_start, (const T *)d_mu0, (const T *)vi->d_occ_tab,
                              (T *)d_mu, (T *)d_occ, (T *)d_ret, (T *)d_mu_t, vi->d_occ_err, N);
        MGDP_HIP(hipGetLastError());
        return 0;
    }
    static int run(mgdp_vi *vi, const int8_t *d_pi, bool ti, const int32_t *d_start, const void *d_mu0, int N,
                   void *d_mu, void *d_occ, void *d_ret, void *d_mu_t) {
        if (ti) return d_mu_t ? launch<true, true>(vi, d_pi, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t)
                              : launch<true, false>(vi, d_pi, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t);
        return d_mu_t ? launch<false, true>(vi, d_pi, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t)
                      : launch<false, false>(vi, d_pi, d_start, d_mu0, N, d_mu, d_occ, d_ret, d_mu_t);
    }
};
template <typename T, typename... Args>
int dispatch_occupancy_t(mgdp_vi *vi, Args... args) {
    const bool nd = vi->d.lava_mode == MGDP_LAVA_NODEATH;
    if (vi->d.slip_p >= 0.0) return nd ? OccupancyF<T, true, true>::run(vi, args...) : OccupancyF<T, true, false>::run(vi, args...);
    return nd ? OccupancyF<T, false, true>::run(vi, args...) : OccupancyF<T, false, false>::run(vi, args...);
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
}  // extern "C++"

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
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    return 0;
}

int mgdp_vi_enable_timing(mgdp_vi *vi, int32_t on) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    if (int rc = timed_collect(vi)) return rc;  // drop launches timed before this call
    vi->timing = on != 0;
    vi->total_ms = 0.0;
    vi->launches = 0;
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
    if (int rc = server_stop(vi)) return rc;  // the server writes the words behind its publish: it has left now
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    account_server_clock(vi);
    *path = (int32_t)vi->h_out[kHoutPath];
    if (counts)
        for (int i = 0; i < 3; ++i) counts[i] = (int64_t)vi->path_counts[i];
    return 0;
}

int mgdp_vi_kernel_time(mgdp_vi *vi, double *total_ms, int64_t *launches) {
    MGDP_CHECK(vi, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(vi->d.device);
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
    if (int rc = timed_collect(vi)) return rc;
    if (total_ms) *total_ms = vi->total_ms;
    if (launches) *launches = vi->launches;
    return 0;
}

}  // extern "C"
