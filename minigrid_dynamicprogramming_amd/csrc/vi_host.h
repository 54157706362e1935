// vi_host.h -- the value-iteration handle: struct mgdp_vi (the ABI's opaque handle) and ViKernels, the
// kernel arguments made of it (make_geo, make_coef), the clock
// of departed servers, the epoch of a host-published launch, and the check of a cells array against the
// model.  Part of the single translation unit vi.hip: included after the device headers, first of the
// host pieces (vi_host.h, vi_host_launch.h, vi_host_serve.h, vi_host_order.h, vi_host_eval.h,
// vi_host_occupancy.h, vi_host_qvalues.h, in this order).
#pragma once

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
    // timing of the dominant kernel (timed.h); a pair's tag: the sweep index of a timed sweep launch, -1 = fused launch
    TimedPool timed;
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
    // mgdp_vi_action_values (vi_qvalues.h): device staging of the host form's Q and opt, grown the same way
    void *d_q_stage[2] = {nullptr, nullptr};
    size_t q_stage_cap[2] = {0, 0};
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

// The epoch of a launch whose result goes to the host-mapped words (never 0: publish() writes a
// device buffer's raw words for epoch 0)
inline unsigned int next_host_epoch(mgdp_vi *vi) {
    if (++vi->epoch == 0u) ++vi->epoch;
    return vi->epoch;
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
