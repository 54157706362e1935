// vi_plan.h -- which value-iteration loop a handle runs, decided once per handle and in one place.
//
// plan_vi(desc, knobs) is pure host C++17 (nothing from HIP): it names the loop family, its size
// parameter, the workgroup shape and the LDS bytes of the fused launch and of the lone-grid server.
// vi.hip maps the plan to kernel pointers once at create (resolve_kernels) and every launch, query and
// name reads the plan; the two numbers that need a device come in through resolve_residency.
// tests/test_vi_plan.py checks the plan on the CPU (tools/vi_plan_dump.cpp).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/mgdp.h"
#include "vi_layout.h"

namespace mgdp {

// One entry per loop family: X(entry, mgdp_vi_variant's string, the string when the lone-grid server
// runs it), plus the two kernel-only tags `generic` and `dk_rows16`.  The kernels take <Loop L, int N>
// as template arguments; N is the family's size.
#define MGDP_LOOPS(X)                                                                                                  \
    X(generic, "generic", "serve")       /* kernel tag: every multi-wave loop in one kernel (the four below) */      \
    X(sa, "sa", "sa")                    /* one thread per (state, action)                  (runs in `generic`) */    \
    X(pair, "pair", "pair")              /* XYD two-sweep step, 3 LDS buffers (fused_fast_xyd2)       (generic) */    \
    X(quad, "quad", "quad")              /* XYD four threads per cell (fused_quad_xyd)                (generic) */    \
    X(xyd_soa, "xyd_soa", "serve")       /* direction-major one thread per cell alone (fused_fast_xyd_soa / */        \
    X(dk_soa, "dk_soa", "serve")         /* fused_fast_dk_soa); grids wider than the workgroup: in `generic` */       \
    X(wave, "wave", "serve_wave")        /* lone XYD grid on one wave, N = 1, 2, 4, 8 cells per lane */               \
    X(xyd_x2, "xyd_x2", "serve")         /* batched XYD, two / four cells per thread (fused_fast_xyd_soa_xn) */       \
    X(xyd_x4, "xyd_x4", "serve")                                                                                       \
    X(xyd_pair2, "xyd_pair2", "serve")   /* batched plain XYD, two adjacent cells per thread, stride 128 * N */       \
    X(wave2, "wave2", "wave2")           /* batched plain XYD, one wave per grid, N cells per lane */                 \
    X(band, "band", "serve_band")        /* ... one wave in column bands of N rows; also a served lone grid */        \
    X(wave2n, "wave2n", "wave2n")        /* ... two waves per grid, N blocks of 64 cells per wave */                  \
    X(mix, "mix", "mix")                 /* ... fp32, N blocks: two waves for the order's long grids, else one */     \
    X(dk_1t, "dk_1t", "dk_1t")           /* batched fp32 DoorKey on one LDS tile (fused_fast_dk_1t) */                \
    X(dk_half, "dk_half", "serve_dk_half") /* DoorKey states over two threads by has_key, plane stride 64 * N */      \
    X(dk_rows, "dk_rows", "dk_rows")     /* batched DoorKey of width 16 on whole-row thread maps */                   \
    X(dk_rows16, "dk_rows", "dk_rows")   /* kernel tag: the same for fp32 16x16 own-rule launches */                  \
    X(serve_ew, "serve_ew", "serve_ew")  /* served lone plain XYD grid, east / west fronts by DPP */                  \
    X(serve_pair, "serve_pair", "serve_pair") /* ... two sweeps per workgroup barrier */                              \
    X(opts, "opts", "opts")              /* NoDeath lava / finite horizon (vi_fused_opts_kernel) */                   \
    X(sweep, "sweep", "sweep")           /* one launch per sweep, staged (vi_sweep_kernel) */                         \
    X(sweep_pipe, "sweep_pipe", "sweep_pipe") /* ... register-pipelined (vi_sweep_pipe_kernel) */
#define MGDP_LOOP_ENUM(e, n, s) e,
#define MGDP_LOOP_NAMES(e, n, s) {n, s},
enum class Loop : int { MGDP_LOOPS(MGDP_LOOP_ENUM) };
inline const char *name(Loop l, bool served) {
    static const char *const names[][2] = {MGDP_LOOPS(MGDP_LOOP_NAMES)};
    return names[(int)l][served ? 1 : 0];
}

// Every MGDP_* run-time knob of the value-iteration handle (read once per mgdp_vi_create).
struct ViKnobs {
    int pair = 0;        // MGDP_PAIR: two-sweep XYD step; measured slower than the one-sweep step on MI355X (VALU chain, not barriers, bound it)
    int quad = 0;        // MGDP_QUAD: four threads per cell; measured slower than one thread per cell (LDS/barrier latency bound it)
    int wave = 1;        // MGDP_WAVE: lone XYD grid on one wave up to this many cells per lane; P = 1 faster (0.10 vs 0.12 us per sweep), 2 even, 4 and 8 slower
    int cpt = 2;         // MGDP_CPT: batched XYD cells per thread (1|2|4); 2 beats 1 by 7-25 % (profiles/r01_cpt/)
    int lone_cpt = 1;    // MGDP_LONE_CPT: a lone grid (latency) keeps one cell per thread unless 2
    int pair2 = 1;       // MGDP_PAIR2: cpt 2 on adjacent-cell pairs (0: fused_fast_xyd_soa_xn)
    int wave2 = 8;       // MGDP_WAVE2: batched plain XYD on one wave per grid up to this many cells per lane (0: off)
    int wave2n = 0;      // MGDP_WAVE2N: two waves per grid; FourRooms x 4096 64-65 us vs 55-56 us on one wave (profiles/r04_w2nab/)
    int mix = 0;         // MGDP_MIX: mixed wave counts (fp32, 2..6 blocks)
    double mix_frac = 0.75;  // MGDP_MIX_FRAC: grids with keys >= this fraction of the longest sweep on two waves
    int band = 0;        // MGDP_BAND: column bands instead of row-major blocks (A/B; off until measured per size)
    int gk = 2;          // MGDP_GK: in-launch reduction 0 never, 1 any B, 2 while resident; past capacity LavaS11N5 x 65536 153 vs 144-145 us (profiles/r05_mix/)
    int bserve = 1;      // MGDP_BSERVE: resident batch server (0 off, 2 also past its resident capacity)
    int bserve_copies = kBreqCopies;  // MGDP_BSERVE_COPIES: request lines the workgroups poll
    int bserve_nap = 1;               // MGDP_BSERVE_NAP: s_sleep(10)s between polls
    int bserve_wait_pub = 1;          // MGDP_BSERVE_WAIT_PUB: the forwarder polls the host only after the publication
    double bserve_prio_frac = 0.0;    // MGDP_BSERVE_PRIO_FRAC: this fraction of the order's longest grids sweeps at a higher issue priority
    int serve_ew = 1;    // MGDP_SERVE_EW: served lone plain XYD grid on fused_serve_xyd
    int serve_pair = 1;  // MGDP_SERVE_PAIR: ... two sweeps per barrier (fused_serve_pair)
    int serve_band = 0;  // MGDP_SERVE_BAND: ... on one wave in column bands (A/B)
    int serve_depth = 1;  // MGDP_SERVE_DEPTH: the pair server reads a fresh request off the goal depth (fused_serve_depth); 0: every request sweeps
    int serve_depth_max = 1 << 20;  // MGDP_SERVE_DEPTH_MAX: the largest depth the form searches out before it hands the request to the pair loop
    int dk_1t = 0;       // MGDP_DK_1T: batched fp32 DoorKey on one LDS tile
    int dk_half = -1;    // MGDP_DK_HALF: -1 = fp64 and lone grids (DoorKey-16 x 65536 fp64 9.9e12 vs 2.8e12 updates/s, fp32 1.90e13 vs 2.22e13; profiles/r02_dk_half/)
    int dk_rows = 1;     // MGDP_DK_ROWS: width-16 DoorKey on whole-row maps (0: fused_fast_dk_soa, half its LDS cycles on bank conflicts)
    int sweep_m = 1;     // MGDP_SWEEP_M: grids staged per workgroup iteration (measured: m > 1 no faster)
    int sweep_grid = 0;  // MGDP_SWEEP_GRID: workgroups of a sweep launch (0: 2048 staged, resident x <= 4 per CU pipelined)
    int sweep_block = 256;  // MGDP_SWEEP_BLOCK
    int sweep_pipe = -1;    // MGDP_SWEEP_PIPE: grids fetched ahead, 0 = staged kernel; -1 = 2 for XYD, 0 for DoorKey (5.38 -> 3.3 TB/s on the pipeline)
    int persistent = 1;     // MGDP_PERSISTENT: resident servers (lone grid, resident batch)
    int chain = 1;          // MGDP_CHAIN: slip batches: run_local -> run_to(K from device memory), one host wait
    int learn_order = 1;    // MGDP_LEARN_ORDER: longest-first dispatch order, +3-6 % (profiles/r05_ab2/)
    int learn_prio = 0;     // MGDP_LEARN_PRIO: issue priority on top of it: nothing or worse
    int order_src = 1;      // MGDP_ORDER: 1 the cells' depth proxy (at load), 2 "learned" the last solve's sweeps, 0 "off"
    int reduce_multi = 1;   // MGDP_REDUCE_MULTI: B > inkernel_max: vi_reduce_multi_kernel
    int inkernel_max = kInKernelReduceMaxB;  // MGDP_INKERNEL_MAX: batches up to this fold {k, dV} in the fused launch itself
    long long serve_idle_us = 100;       // MGDP_SERVE_IDLE_US: the server leaves after this long without a request
    long long serve_life_us = 2000000;   // MGDP_SERVE_LIFE_US
    int serve_pollers = 1;   // MGDP_SERVE_POLLERS: waves polling the request word (1 measured 0.2-0.4 us faster than 4)
    int serve_poll_dma = 1;  // MGDP_SERVE_POLL_DMA: polls land in an LDS mailbox, several in flight (0: one at a time)
};

// How a knob's text becomes its value: atoi / atof / atoll as ever, then the clamp
enum class KnobKind { integer, flag, clamp, at_least, real, real_clamp, micros, two_or_one, block64, order };
struct KnobSpec {
    const char *env;
    int ViKnobs::*i;
    double ViKnobs::*f;
    long long ViKnobs::*ll;
    KnobKind kind;
    double lo, hi;
};
inline const KnobSpec *knob_table(int *n) {
    using K = ViKnobs;
    using T = KnobKind;
    static const KnobSpec t[] = {
        {"MGDP_PAIR", &K::pair, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_QUAD", &K::quad, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_WAVE", &K::wave, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_CPT", &K::cpt, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_LONE_CPT", &K::lone_cpt, nullptr, nullptr, T::two_or_one, 0, 0},
        {"MGDP_PAIR2", &K::pair2, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_WAVE2", &K::wave2, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_WAVE2N", &K::wave2n, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_MIX", &K::mix, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_MIX_FRAC", nullptr, &K::mix_frac, nullptr, T::real, 0, 0},
        {"MGDP_BAND", &K::band, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_GK", &K::gk, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_BSERVE", &K::bserve, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_BSERVE_COPIES", &K::bserve_copies, nullptr, nullptr, T::clamp, 1, kBreqCopies},
        {"MGDP_BSERVE_NAP", &K::bserve_nap, nullptr, nullptr, T::clamp, 0, 64},
        {"MGDP_BSERVE_WAIT_PUB", &K::bserve_wait_pub, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_BSERVE_PRIO_FRAC", nullptr, &K::bserve_prio_frac, nullptr, T::real_clamp, 0.0, 1.0},
        {"MGDP_SERVE_EW", &K::serve_ew, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_SERVE_PAIR", &K::serve_pair, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_SERVE_BAND", &K::serve_band, nullptr, nullptr, T::integer, 0, 0},
        {"MGDP_SERVE_DEPTH", &K::serve_depth, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_SERVE_DEPTH_MAX", &K::serve_depth_max, nullptr, nullptr, T::at_least, 1, 0},
        {"MGDP_DK_1T", &K::dk_1t, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_DK_HALF", &K::dk_half, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_DK_ROWS", &K::dk_rows, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_SWEEP_M", &K::sweep_m, nullptr, nullptr, T::at_least, 1, 0},
        {"MGDP_SWEEP_GRID", &K::sweep_grid, nullptr, nullptr, T::at_least, 1, 0},
        {"MGDP_SWEEP_BLOCK", &K::sweep_block, nullptr, nullptr, T::block64, 64, 256},
        {"MGDP_SWEEP_PIPE", &K::sweep_pipe, nullptr, nullptr, T::clamp, 0, 4},
        {"MGDP_PERSISTENT", &K::persistent, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_CHAIN", &K::chain, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_LEARN_ORDER", &K::learn_order, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_LEARN_PRIO", &K::learn_prio, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_ORDER", &K::order_src, nullptr, nullptr, T::order, 0, 0},
        {"MGDP_REDUCE_MULTI", &K::reduce_multi, nullptr, nullptr, T::flag, 0, 0},
        {"MGDP_INKERNEL_MAX", &K::inkernel_max, nullptr, nullptr, T::at_least, 0, 0},
        {"MGDP_SERVE_IDLE_US", nullptr, nullptr, &K::serve_idle_us, T::micros, 1, 0},
        {"MGDP_SERVE_LIFE_US", nullptr, nullptr, &K::serve_life_us, T::micros, 1, 0},
        {"MGDP_SERVE_POLLERS", &K::serve_pollers, nullptr, nullptr, T::at_least, 1, 0},
        {"MGDP_SERVE_POLL_DMA", &K::serve_poll_dma, nullptr, nullptr, T::flag, 0, 0},
    };
    *n = (int)(sizeof(t) / sizeof(t[0]));
    return t;
}
inline void set_knob(ViKnobs &k, const KnobSpec &s, const char *v) {
    switch (s.kind) {
    case KnobKind::integer: k.*s.i = std::atoi(v); break;
    case KnobKind::flag: k.*s.i = std::atoi(v) != 0; break;
    case KnobKind::clamp: k.*s.i = std::min((int)s.hi, std::max((int)s.lo, std::atoi(v))); break;
    case KnobKind::at_least: k.*s.i = std::max((int)s.lo, std::atoi(v)); break;
    case KnobKind::real: k.*s.f = std::atof(v); break;
    case KnobKind::real_clamp: k.*s.f = std::min(s.hi, std::max(s.lo, std::atof(v))); break;
    case KnobKind::micros: k.*s.ll = std::max((long long)s.lo, std::atoll(v)); break;
    case KnobKind::two_or_one: k.*s.i = std::atoi(v) == 2 ? 2 : 1; break;
    case KnobKind::block64: k.*s.i = std::min((int)s.hi, std::max((int)s.lo, std::atoi(v) / 64 * 64)); break;
    case KnobKind::order: k.*s.i = std::strcmp(v, "learned") == 0 ? 2 : (std::strcmp(v, "off") == 0 ? 0 : 1); break;
    }
}
// By name (tests, tools): false if no knob has that name
inline bool set_knob(ViKnobs &k, const char *env, const char *v) {
    int n = 0;
    const KnobSpec *t = knob_table(&n);
    for (int i = 0; i < n; ++i)
        if (std::strcmp(t[i].env, env) == 0) {
            set_knob(k, t[i], v);
            return true;
        }
    return false;
}
inline ViKnobs read_knobs() {
    ViKnobs k;
    int n = 0;
    const KnobSpec *t = knob_table(&n);
    for (int i = 0; i < n; ++i)
        if (const char *v = std::getenv(t[i].env)) set_knob(k, t[i], v);
    return k;
}

struct ViPlan {
    // the fused launch: the family it reports, the vi_fused_kernel instantiation <kern, n> that runs it
    Loop loop = Loop::generic, kern = Loop::generic;
    int n = 0;                   // P, HB, PW, HWs / 64 or HWs / 128 (0: the family has no size)
    // the lone-grid server (B == 1): the same for vi_serve_kernel
    Loop serve_loop = Loop::generic, serve_kern = Loop::generic;
    int serve_n = 0;
    int block = 256;             // workgroup threads of the fused launch and the server
    int HWs = 0, Ss = 0;         // see Geo
    int nbuf = 2;                // LDS V buffers of the usual layout
    int cpt = 1;                 // cells per thread
    int lds = 0, serve_lds = 0;  // dynamic LDS bytes: fused launch, lone-grid server
    int lds_base = 0;            // the usual layout at the base stride (create refuses > 160 KiB)
    bool opts = false;           // NoDeath lava / finite horizon
    bool pair = false, quad = false;  // Geo::pair / quad
    int wave2 = 0;               // blocks of 64 cells of a one-wave-per-grid batch (wave2, wave2n, mix, band; bserve's P)
    bool serve_shape = false;    // a lone grid the server can hold (serve_eligible without MGDP_PERSISTENT)
    bool wants_gk = false;       // a wave2-family launch: the in-launch reduction if resident (resolve_residency)
    bool wants_bserve = false;   // ... and the resident batch server may run it
    int sweep_m = 1, sweep_grid = 2048, sweep_block = 256, sweep_pipe = 2;  // the sweep method's launches
    int B = 0, gk_mode = 2;      // the batch and MGDP_GK, for resolve_residency
    // resolve_residency (needs the device):
    bool gk = false;             // the in-launch reduction is on
    bool wt = false;             // Geo::wt: the batch is resident at once (write-through exit stores)
    int gk_capacity = 0;         // resident workgroups of the fused kernel
    int bserve_cap = 0;          // resident workgroups of vi_bserve_kernel (0: no batch server)
    bool bserve_any = false;     // also batches past that capacity (MGDP_BSERVE=2)
};

// The one place where the precedence among the variants is written.  Each family states its
// eligibility once; `plain` is the prefix they share.
inline ViPlan plan_vi(const mgdp_vi_desc &d, const ViKnobs &kn) {
    ViPlan p;
    p.B = d.B;
    p.gk_mode = kn.gk;
    const bool xyd = d.model == MGDP_MODEL_XYD, dk = d.model == MGDP_MODEL_DOORKEY;
    const bool fused = d.method == MGDP_METHOD_FUSED, cell = d.mapping == MGDP_MAP_CELL;
    const bool det = d.slip_p < 0.0, lone = d.B == 1, f32 = d.dtype == MGDP_F32;
    const int HW = d.W * d.H, HWp = (int)round_up(HW, 16), per_cell = xyd ? 4 : 16, S = HW * per_cell;
    const int tsize = f32 ? 4 : 8;
    auto stride = [&](int HWs) { p.HWs = HWs; p.Ss = per_cell * HWs; };
    stride(HW <= 1024 ? (int)round_up(HW, 64) : HW);

    p.opts = d.horizon > 0 || d.lava_mode != MGDP_LAVA_TERMINAL;
    // the options kernel runs the direction-major path only
    p.pair = xyd && cell && HW <= 1024 && kn.pair && !p.opts;
    p.quad = xyd && cell && HW <= 1024 && !kn.pair && kn.quad && 4 * HW <= 1024 && !p.opts;
    p.nbuf = p.pair ? 3 : 2;
    p.lds_base = smem_layout(p.Ss, HWp, tsize, p.nbuf).total();

    int wave_p = 0, wave2n = 0, band = 0;
    bool mix = false, serve_ew = false, serve_pair = false, dk1t = false, dkhalf = false, dkrow = false;
    if (cell) {
        // fused: one workgroup per grid, one thread per cell when the grid has <= 1024 cells
        p.block = (int)std::min<int64_t>(1024, round_up(HW * (p.quad ? 4 : 1), 64));
        const bool plain = fused && !p.pair && !p.quad && !p.opts;  // the shared prefix of every rule below
        const int hb = band_rows(d.W, d.H);
        // a lone XYD grid of <= 64 * MGDP_WAVE cells on ONE wave, P = 1, 2, 4 or 8 cells per lane
        if (lone && xyd && plain && HW <= 64 * std::min(kn.wave, 8)) {
            wave_p = 1;
            while (64 * wave_p < HW) wave_p *= 2;
            stride(64 * wave_p);
            p.block = 64;
        }
        // batched XYD grids: N cells per thread divides the waves per grid by N
        const int cpt = wave_p ? 1 : lone ? kn.lone_cpt : kn.cpt;
        if ((cpt == 2 || cpt == 4) && xyd && plain && HW <= 1024) {
            p.cpt = cpt;
            p.block = (int)round_up((HW + cpt - 1) / cpt, 64);
            stride(cpt * p.block);
        }
        // batched deterministic XYD grids: one wave per grid, up to MGDP_WAVE2 cells per lane
        const int P2 = (HW + 63) / 64;
        if (!lone && xyd && plain && det && P2 <= std::min(kn.wave2, 8)) {
            p.wave2 = P2;
            p.cpt = 1;
            p.block = 64;
            stride((int)round_up(HW, 64));
            // ... on two waves (grids of >= 3 blocks), mixed wave counts (fp32, 2..6 blocks), or column bands
            if (kn.wave2n && P2 >= 3) wave2n = (P2 + 1) / 2;
            mix = kn.mix && !wave2n && f32 && P2 >= 2 && P2 <= 6;
            if (wave2n || mix) p.block = 128;
            if (kn.band && !wave2n && !mix && hb >= 1 && hb <= 8) band = hb;
            p.wants_gk = true;
            p.wants_bserve = kn.bserve != 0 && !band && !mix && !wave2n;
            p.bserve_any = kn.bserve == 2;
        }
        // the served lone deterministic XYD grid: east / west fronts by DPP, <= 4 waves (one dword of
        // stop flags); the two-plane padded tiles must fit the usual V buffers
        const bool lone_plain = lone && xyd && plain && det;
        serve_ew = kn.serve_ew && lone_plain && !wave_p && p.cpt == 1 && p.block <= 256 && p.HWs >= p.block &&
                   2 * p.HWs >= 3 * serve_ew_padw(d.W);
        // ... with two sweeps per workgroup barrier: its two four-plane tiles take the first V buffers
        // (nbuf raised to hold them)
        if (serve_ew && kn.serve_pair) {
            const int need = 2 * serve_pair_tile_elems(p.HWs, d.W);
            const int nbuf = std::max(2, (need + p.Ss - 1) / p.Ss);
            if (smem_layout(p.Ss, HWp, tsize, nbuf).total() <= 64 * 1024) {
                serve_pair = true;
                p.nbuf = nbuf;
            }
        }
        // ... on ONE wave in column bands instead (no barrier, no LDS tile); the plane stride stays
        if (kn.serve_band && lone_plain && hb >= 1 && hb <= 8) {
            band = hb;
            serve_ew = serve_pair = false;
            p.nbuf = 2;
            wave_p = 0;
            p.cpt = 1;
            p.block = 64;
        }
        // DoorKey: one LDS tile (fp32 batches), states split by has_key (fp64 and lone grids unless
        // MGDP_DK_HALF says otherwise, <= 512 cells), whole-row maps (batches of width 16)
        const bool dk_plain = dk && fused && !p.opts;
        if (kn.dk_1t && !lone && dk_plain && f32 && HW <= p.block) {
            dk1t = true;
            p.nbuf = 1;
        }
        if ((kn.dk_half < 0 ? (!f32 || lone) : kn.dk_half != 0) && !dk1t && dk_plain && HW <= 512) {
            dkhalf = true;
            stride((int)round_up(HW, 64));
            p.block = 2 * p.HWs;
        }
        if (kn.dk_rows && !dk1t && !dkhalf && !lone && dk_plain && det && !p.pair && !p.quad && d.W == 16 && HW <= 1024) {
            dkrow = true;
            stride((int)round_up(HW, 64));
            p.block = p.HWs;
        }
    } else {  // MAP_SA: 8 lanes per state, a lone grid gets the widest workgroup
        p.block = lone ? 1024 : 256;
        while (p.block > 64 && p.block / 2 >= S * 8) p.block /= 2;
    }

    // the vi_fused_kernel instantiation and its LDS bytes
    p.lds = smem_layout(p.Ss, HWp, tsize, p.nbuf).total();
    if (xyd && cell) {
        if (wave_p == 1 || wave_p == 2 || wave_p == 4 || wave_p == 8) p.kern = Loop::wave, p.n = wave_p;
        if (p.cpt == 2) p.kern = det && kn.pair2 ? Loop::xyd_pair2 : Loop::xyd_x2, p.n = det && kn.pair2 ? p.HWs / 128 : 0;
        if (p.cpt == 4) p.kern = Loop::xyd_x4, p.n = 0;
    }
    if (dk && cell && det) {
        if (dk1t) p.kern = Loop::dk_1t;
        else if (dkhalf) p.kern = Loop::dk_half, p.n = p.HWs / 64;
        else if (dkrow) p.kern = Loop::dk_rows, p.lds = dkrow_smem_bytes(HWp, p.HWs, tsize);
    }
    if (cell && p.kern == Loop::generic && !p.pair && !p.quad && HW <= p.block) p.kern = xyd ? Loop::xyd_soa : Loop::dk_soa;
    if (xyd && cell && det) {
        if (mix) p.kern = Loop::mix, p.n = p.wave2, p.lds = mix_smem_bytes(HWp, d.W, p.wave2, tsize);
        else if (wave2n) p.kern = Loop::wave2n, p.n = wave2n, p.lds = wave2n_smem_bytes(HWp, d.W, 2 * wave2n, tsize);
        else if (band) p.kern = Loop::band, p.n = band, p.lds = band_smem_bytes(HWp);
        else if (p.wave2) p.kern = Loop::wave2, p.n = p.wave2, p.lds = wave2_smem_bytes(HWp, d.W, p.wave2, tsize);
    }
    // the family reported: the instantiation, or what runs inside the generic kernel
    p.loop = p.kern != Loop::generic ? p.kern
             : !cell                 ? Loop::sa
             : p.pair                ? Loop::pair
             : p.quad                ? Loop::quad
                                     : (dk ? Loop::dk_soa : Loop::xyd_soa);

    // the lone-grid server: its loop, instantiation and LDS bytes (the usual layout)
    p.serve_shape = !p.opts && fused && lone && cell && (HW <= p.cpt * p.block || wave_p || band) && !p.pair && !p.quad;
    p.serve_lds = smem_layout(p.Ss, HWp, tsize, p.nbuf).total();
    p.serve_loop = p.loop;
    if (p.kern == Loop::wave) p.serve_kern = Loop::wave, p.serve_n = p.n;
    if (xyd && cell) {
        if (p.cpt == 2) p.serve_kern = p.serve_loop = Loop::xyd_x2, p.serve_n = 0;
        if (det && serve_ew) p.serve_kern = p.serve_loop = serve_pair ? Loop::serve_pair : Loop::serve_ew, p.serve_n = 0;
        if (det && band) p.serve_kern = p.serve_loop = Loop::band, p.serve_n = band;
    }
    if (dk && cell && det && dkhalf) p.serve_kern = p.serve_loop = Loop::dk_half, p.serve_n = p.HWs / 64;

    // the sweep method
    p.sweep_m = kn.sweep_m;
    // keep the staged group within the LDS budget (two groups per CU at least)
    while (p.sweep_m > 1 && sweep_smem_bytes(S, HWp, tsize, p.sweep_m) > 80 * 1024) --p.sweep_m;
    p.sweep_grid = kn.sweep_grid > 0 ? kn.sweep_grid : 2048;
    p.sweep_block = kn.sweep_block;
    p.sweep_pipe = kn.sweep_pipe >= 0 ? kn.sweep_pipe : (dk ? 0 : 2);
    if (HW > 1024 || !cell || sweep_pipe_smem_bytes(S, HW, p.HWs, HWp, tsize) > 160 * 1024)
        p.sweep_pipe = 0;  // one thread per cell: grids of <= 1024 cells
    if (!fused) p.loop = cell && p.sweep_pipe ? Loop::sweep_pipe : Loop::sweep;
    else if (p.opts) p.loop = Loop::opts;
    return p;
}

// The device-dependent step: resident workgroups per CU of the fused kernel and of the batch
// server (0 where the query failed or was not needed), CUs of the device.
inline void resolve_residency(ViPlan &p, int fused_per_cu, int bserve_per_cu, int cus) {
    if (!p.wants_gk) return;
    p.gk_capacity = fused_per_cu * cus;
    p.gk = p.gk_mode == 1 || (p.gk_mode == 2 && p.B <= p.gk_capacity);
    p.wt = p.gk_capacity > 0 && p.B <= p.gk_capacity;
    if (p.wants_bserve && (p.gk || p.bserve_any)) p.bserve_cap = bserve_per_cu * cus;
}

// What mgdp_vi_variant / mgdp_vi_kernel_name report; served: the lone-grid server is on
inline const char *variant_name(const ViPlan &p, bool served) {
    return served ? name(p.serve_loop, true) : name(p.loop, false);
}
inline const char *kernel_name(const ViPlan &p, bool served) {
    switch (p.loop) {
    case Loop::opts: return "vi_fused_opts_kernel";
    case Loop::sweep: return "vi_sweep_kernel";
    case Loop::sweep_pipe: return "vi_sweep_pipe_kernel";
    default: return served ? "vi_serve_kernel" : "vi_fused_kernel";
    }
}

}  // namespace mgdp
