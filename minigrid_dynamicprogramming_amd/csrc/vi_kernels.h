// vi_kernels.h -- the value-iteration kernels: fused solve, persistent lone-grid server,
// options kernel, reduce kernel, per-sweep HBM kernel.
// Part of the single translation unit vi.hip (included in order: vi_model.h, vi_loops.h,
// vi_kernels.h); see vi.hip for the DP semantics and the data layout.
#pragma once

namespace mgdp {
// vi_fused_kernel / vi_serve_kernel instantiations are named <Loop L, int N> (vi_plan.h): the loop
// family and its size.  Notes on what the tags buy:
//  * Loop::generic also holds the cell-major, pair and quad loops, and a kernel's VGPR budget is that
//    of its hungriest path: Loop::xyd_soa / dk_soa (the direction-major one-thread-per-cell path
//    alone) strip them, which is what sets the batched kernels' occupancy.
//  * Loop::dk_rows16 is dk_rows for exactly 16x16 cells (DoorKey-16x16: 256 threads, plane stride known
//    at compile time, so one LDS base register serves every tile access) and own-rule launches only
//    (one copy of the sweep loops: the run_to copy kept values live across both).  Both are what let
//    the fp32 loop fit 80 VGPRs -- 6 waves per SIMD -- with no scratch (round 5's 6-wave build spilled
//    76 B per thread).
//  * Loop::mix (fp32, N = 2..6 blocks of 64 cells, 128-thread workgroups): the first Geo::nmix
//    workgroups of the learned dispatch order (the grids whose previous solve ran longest) sweep on two
//    waves (fused_wave2n_xyd, PW = ceil(N / 2) blocks each), every other grid on one (fused_wave2_xyd;
//    its second wave leaves at once).  For batches whose launch is set by a long tail of slow grids (an
//    8-way LavaS11N5 shard: median 24 sweeps, max 47): splitting a long grid's sweep chain over two
//    waves shortens the tail.
//  * Loop::serve_ew falls back to fused_fast_xyd_soa for a grid whose wave edges do not allow it.
__host__ __device__ constexpr bool loop_is_dkrow(Loop l) { return l == Loop::dk_rows || l == Loop::dk_rows16; }
__host__ __device__ constexpr bool loop_is_serve_ew(Loop l) { return l == Loop::serve_ew || l == Loop::serve_pair; }
// every instantiation but the generic one and the lone wave runs the direction-major path alone
__host__ __device__ constexpr bool loop_is_soa_only(Loop l) { return l != Loop::generic && l != Loop::wave; }
// Minimum waves per SIMD the one-wave kernels are compiled for.  Left alone, the fp32 P <= 2
// variants (LavaS11N5: 121 cells) take 57 VGPRs but 106 SGPRs, and the SGPRs cap them at 7 waves
// per SIMD (28 workgroups / CU, 7168 grids resident): 8 makes the compiler fit 8 waves' SGPRs too
// (78 SGPRs, 32 / CU, 8192 resident -- an 8-way shard of LavaS11N5 x 65536 then fits the
// launch-wide rule in one launch: 89 -> 60 us per solve; the whole 65536 batch +4.5 %).  Same for
// fp64 P = 1 (57 VGPRs); the other variants are VGPR-bound at <= 6 waves.  Batches at the SGPR-bound
// residency also hit a dispatcher limit the occupancy API does not see: LavaS11N5 x 7168 at 28 / CU
// took 199 us (waiting grids ran to the cap) against 57 us at 32 / CU (profiles/r03_w8/).
// Tried: fp32 P = 4 (Empty-16) at 6 waves instead of its 91-VGPR 5, and a minimum for the
// two-waves-per-grid kernels (wave2n); neither was kept.
// Minimum waves per SIMD of fp32 fused_dk_rows: round 5's 6 (80 VGPRs and 76-80 B of scratch, 6 grids per
// CU) measured 1950-1960 vs 1992-1996 us per DoorKey-16 x 65536 solve at 5, neutral at 8192 grids
// (profiles/r05_dkw6/), but its spill stores doubled the launch's HBM writes.  Now: the 16x16 own-rule
// variant (Loop::dk_rows16) at 6 waves, 80 VGPRs, no scratch; the general one at 5 (96 VGPRs, no scratch).
template <typename T>
__host__ __device__ constexpr int wave2_min_waves(Loop l, int n) {
    return l == Loop::dk_rows     ? (sizeof(T) == 4 ? 5 : 1)  // fp64 at 6 waves spills 492 B
           : l == Loop::dk_rows16 ? (sizeof(T) == 4 ? 6 : 1)
           : (l == Loop::mix && n <= 2) ? 8
           : (l == Loop::wave2 && n <= (sizeof(T) == 4 ? 2 : 1)) ? 8
                                                                  : 1;
}
// Loop::dk_half: batched DoorKey, a cell's states split over two threads by has_key (fused_dk_half;
// workgroup = 2 * HWs threads), plane stride HWs = 64 * N known at compile time.
template <typename T, int MODEL> struct TopoOf { using type = XydTopo<T>; };
template <typename T> struct TopoOf<T, MGDP_MODEL_DOORKEY> { using type = DkTopo; };

// ------------------------------------------------------------------------------------------------
// The per-grid protocol every solving kernel follows: resume {k, dV}, apply fixed-point completion,
// test for work, sweep, record the result.  Its pieces, each said once:
// ------------------------------------------------------------------------------------------------
// Fixed-point completion: a grid whose last sweep changed nothing (|dV| = 0 exactly, so
// V_k == V_{k-1} bit for bit) reproduces V_k at every later sweep (a Jacobi sweep is a function
// of V alone), and pi_{k'} = argmax on V_{k'-1} = pi_k: it is at sweep k_target already, with
// dV 0.  Only its sweep count moves (the reduce kernel reads it).
__device__ __forceinline__ bool grid_complete_at(int k, double dvl, int k_target) {
    return k_target > k && k > 0 && dvl == 0.0;
}
// own rule (k_target < 0): not yet below tol and under the sweep cap; run_to: short of k_target
__device__ __forceinline__ bool grid_has_work(const Geo &geo, int k, double dvl, int k_target) {
    return k_target < 0 ? (!(k > 0 && dvl < geo.tol) && k < geo.max_sweeps) : (k < k_target);
}
// The grid's record: its sweep count (also the learned dispatch order's input) and last |dV|.
__device__ __forceinline__ void record_grid(const Geo &geo, int32_t *kenv, double *dvenv, int e, int k, double dvl,
                                            bool writer) {
    if (writer) {
        kenv[e] = k;
        if (geo.kexec) geo.kexec[e] = k;
        dvenv[e] = dvl;
    }
}
// A solve's early publication, from inside its loop (before the pi pass and the exit stores): a
// launch of one grid publishes {k, dV, k} itself; a served solve publishes tagged with its request.
template <bool SERVED>
__device__ __forceinline__ void publish_solve(unsigned long long *host_out, int kk, double dv, unsigned int epoch,
                                              bool lone, bool writer) {
    if (SERVED) {
        if (writer) {
#ifdef MGDP_SERVE_TRACE
            // the stamps are taken in front of the publish and stored behind it, so that "loop left ->
            // publish" is the plain build's path; the host waits for word 9, stored last
            const unsigned long long c_pub = __builtin_amdgcn_s_memtime(), t_pub = __builtin_amdgcn_s_memrealtime();
#endif
            publish_tagged(host_out, kk, dv, epoch);
#ifdef MGDP_SERVE_TRACE
            // the pair loop's stamps of this solve (fused_serve_pair stored them just now), words 18..23
            for (int i = 0; i < 6; ++i)
                __hip_atomic_store(host_out + 18 + i, g_pair_trace[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_out + 15, c_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_out + 9, t_pub, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
        }
    } else if (lone && writer) {
        publish(host_out, (unsigned long long)kk, (unsigned long long)__double_as_longlong(dv),
                (unsigned long long)kk, epoch);
    }
}
// A loop's two instantiations -- own rule (LOCAL) and run-to -- from one call site: the call is written
// once, with OWN_RULE as its LOCAL argument.  Tried: a constexpr-bool dispatcher taking a generic lambda
// (by_rule(own, [&](auto r) { loop<T, r.value>(...); })); the closure sits between the kernel's
// __restrict__ arguments and the loop until after inlining, and registers moved in 130 kernels.
// The macro expands to the twin call as it was written out before.  Undefined below fused_grid.
#define MGDP_BY_RULE(own, ...)               \
    do {                                     \
        if (own) {                           \
            constexpr bool OWN_RULE = true;  \
            __VA_ARGS__;                     \
        } else {                             \
            constexpr bool OWN_RULE = false; \
            __VA_ARGS__;                     \
        }                                    \
    } while (0)

// What a persistent lone-grid server resolves once per staged grid and hands to every solve
// (vi_serve_kernel; a launch passes none).
template <typename T, int MODEL>
struct ServeCtx {
    typename TopoOf<T, MODEL>::type topo;  // this thread's cell topology (Loop::generic, serve_ew, serve_pair)
    ServePairTopo<T> sp;                   // Loop::serve_pair: its own per-grid constants
    int ew;  // Loop::serve_ew / serve_pair: 0 = the grid falls back, 1 = the served loop, 2 = the same, first
             // solve of the grid (tiles to clear)
    // Loop::serve_pair, the depth form (vi_serve_depth.h): the grid's masks, the launch's two constants
    // (depth_max 0: MGDP_SERVE_DEPTH=0, every request sweeps) and the path the last request took
    // (mgdp_vi_serve_path: 0 swept, 1 depth form, 2 depth form abandoned, then swept)
    ServeDepthTopo depth;
    int depth_max, depth_ktol;
    mutable int path;
};

// One grid of a fused launch or of a served request, for every Loop family: prologue (resume, learned
// priority, fixed-point completion, work test), the family's section (its LDS staging and its loop),
// epilogue (the record).  Returns whether the grid swept (and so published, if it publishes itself).
// gk: the launch-wide rule's counter tree (wave2-family launches); sc: the server's context (SERVED only).
template <typename T, int MODEL, bool SLIP, int MAP, bool SERVED = false, Loop L = Loop::generic, int N = 0>
__device__ __forceinline__ bool fused_grid(const Geo &geo, const Coef<T> &cf, const uint8_t *__restrict__ cells,
                                           T *__restrict__ V, int8_t *__restrict__ pi, int32_t *__restrict__ kenv,
                                           double *__restrict__ dvenv, unsigned long long *__restrict__ host_out,
                                           int k_target, int fresh, bool lone, unsigned int epoch, int e,
                                           int &k, double &dvl, unsigned long long *gk = nullptr,
                                           const ServeCtx<T, MODEL> *sc = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem LY = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), geo.nbuf);
    T *V0 = reinterpret_cast<T *>(smem);
    T *V1 = reinterpret_cast<T *>(smem + LY.v_bytes);
    int8_t *pis = reinterpret_cast<int8_t *>(smem + LY.pi_off());
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + LY.cells_off());
    T *slots = reinterpret_cast<T *>(smem + LY.slots_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + LY.flags_off());

    // workgroup-uniform: in SGPRs (as VGPRs they stayed live across the sweep loops -- a register
    // pair the batched DoorKey loop at 80 VGPRs had to spill to scratch)
    k = __builtin_amdgcn_readfirstlane(fresh ? 0 : kenv[e]);
    {
        const long long b = fresh ? 0ll : __double_as_longlong(dvenv[e]);
        const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)b);
        const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(b >> 32));
        dvl = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    if (geo.kprio[2] > 0 && k_target < 0) {
        // learned priority: the grids that ran longest last time get the SIMDs' issue slots first, so
        // the launch's critical path (its longest grids) is not stretched by the short ones
        const int kp = geo.kexec[e];
        if (kp >= geo.kprio[0]) __builtin_amdgcn_s_setprio(3);
        else if (kp >= geo.kprio[1]) __builtin_amdgcn_s_setprio(2);
        else if (kp >= geo.kprio[2]) __builtin_amdgcn_s_setprio(1);
    }
    if (grid_complete_at(k, dvl, k_target)) {
        if (threadIdx.x == 0) kenv[e] = k_target;
        k = k_target;
        return false;
    }
    // (grid_has_work, written out: through the helper, registers moved in 79 of these kernels)
    const bool work = k_target < 0 ? (!(k > 0 && dvl < geo.tol) && k < geo.max_sweeps) : (k < k_target);
    if (!work) return false;

    const bool own = k_target < 0;  // the grid's own stopping rule; else run to sweep k_target
    const long long vb = (long long)e * geo.S;
    const GkCtx gkc{gk, epoch, e, geo.B, host_out};  // the in-launch reduction of an own-rule launch (gk != nullptr)
    // The thread that publishes and records is thread 0.  fused_dk_rows re-derives the thread index after
    // its sweep loop (late_tid) and returns it in tl: nothing behind that loop reads threadIdx.x.
    int tl = 0;
    auto writer = [&]() { return loop_is_dkrow(L) ? tl == 0 : threadIdx.x == 0; };
    auto done = [&](int kk, double dv) { publish_solve<SERVED>(host_out, kk, dv, epoch, lone, writer()); };

    if constexpr (L == Loop::mix) {  // two waves for the first nmix workgroups, one for the rest
        static_assert(MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL && !SERVED, "mix: batched plain XYD");
        constexpr int P = N, PW = (P + 1) / 2;
        uint8_t *cl2 = smem + 256;
        copy16(cl2, cells + (long long)e * geo.HWp, geo.HWp);
        T *tile = reinterpret_cast<T *>(smem + wave2_tile_off(geo.HWp));
        if ((int)blockIdx.x < geo.nmix) {  // workgroup-uniform: both waves are here
            __syncthreads();
            MGDP_BY_RULE(own,
                         fused_wave2n_xyd<T, OWN_RULE, PW>(geo, cf, cl2, tile, V + vb, V + vb, pi + vb, k, k_target, dvl, done, gkc));
        } else {  // wave 0 alone (vi_fused_kernel let wave 1 go)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            MGDP_BY_RULE(own,
                         fused_wave2_xyd<T, OWN_RULE, P>(geo, cf, cl2, tile, V + vb, V + vb, pi + vb, k, k_target, dvl, done, gkc));
        }
    } else if constexpr (L == Loop::wave2n) {  // two waves per grid: cells, then two N/S tiles (wave2n_*)
        static_assert(MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL && !SERVED, "wave2n: batched plain XYD");
        uint8_t *cl2 = smem + 256;
        copy16(cl2, cells + (long long)e * geo.HWp, geo.HWp);
        __syncthreads();
        T *tile = reinterpret_cast<T *>(smem + wave2_tile_off(geo.HWp));
        MGDP_BY_RULE(own,
                     fused_wave2n_xyd<T, OWN_RULE, N>(geo, cf, cl2, tile, V + vb, V + vb, pi + vb, k, k_target, dvl, done, gkc));
    } else if constexpr (L == Loop::band) {  // LDS: slots, then the cells (no tile); served: the server's staged cells
        static_assert(MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL, "band: plain XYD");
        uint8_t *cl2 = SERVED ? cl : smem + 256;
        if (!SERVED) {
            copy16(cl2, cells + (long long)e * geo.HWp, geo.HWp);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: its LDS writes are ordered
        }
        MGDP_BY_RULE(own, fused_band_xyd<T, OWN_RULE, N>(geo, cf, cl2, V + vb, V + vb, pi + vb, k, k_target, dvl, done, gkc));
    } else if constexpr (L == Loop::wave2) {  // its own LDS layout (wave2_*): cells, then the N/S tile
        static_assert(MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL && !SERVED, "wave2: batched plain XYD");
        uint8_t *cl2 = smem + 256;
        copy16(cl2, cells + (long long)e * geo.HWp, geo.HWp);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: its LDS writes are ordered
        T *tile = reinterpret_cast<T *>(smem + wave2_tile_off(geo.HWp));
        // Irregular: a third instantiation.  A resident own-rule launch (gk: with the in-launch reduction;
        // geo.wt: a protocol launch, without) writes its exit stores through the L2 (WT); the plain
        // own-rule instantiation takes no GkCtx, so it holds no counter-tree code.
        if (own && (gk != nullptr || geo.wt))
            fused_wave2_xyd<T, true, N, true>(geo, cf, cl2, tile, V + vb, V + vb, pi + vb, k, k_target, dvl, done, gkc);
        else
            MGDP_BY_RULE(own,
                         fused_wave2_xyd<T, OWN_RULE, N>(geo, cf, cl2, tile, V + vb, V + vb, pi + vb, k, k_target, dvl, done));
    } else if constexpr (loop_is_dkrow(L)) {  // its own LDS layout (dkrow_*): slots, flags, row map, cells, tiles
        static_assert(MODEL == MGDP_MODEL_DOORKEY && !SLIP && MAP == MGDP_MAP_CELL && !SERVED, "dkrow: batched DoorKey");
        uint8_t *cl2 = smem + dkrow_cells_off();
        copy16(cl2, cells + (long long)e * geo.HWp, geo.HWp);
        __syncthreads();
        T *tiles = reinterpret_cast<T *>(smem + dkrow_tile_off(geo.HWp));
        T *slots2 = reinterpret_cast<T *>(smem);
        // Irregular: dk_rows16 has only the own-rule instantiation (the host picks Loop::dk_rows for run_to)
        if constexpr (L == Loop::dk_rows16)
            fused_dk_rows<T, true, 256>(geo, cf, cl2, tiles, slots2, smem + 256, smem + 320, V + vb, V + vb, pi + vb, k, k_target, dvl,
                                        done, tl);
        else
            MGDP_BY_RULE(own,
                         fused_dk_rows<T, OWN_RULE>(geo, cf, cl2, tiles, slots2, smem + 256, smem + 320, V + vb, V + vb, pi + vb,
                                                         k, k_target, dvl, done, tl));
    } else {
        // The layout of smem_layout: Loop::wave, the direction-major loops (one thread per cell, or CPT
        // cells: xyd_pair2 / xyd_x2 / xyd_x4) and, for Loop::generic alone, the cell-major paths.
        constexpr bool SOA_ONLY = loop_is_soa_only(L);
        constexpr int CPT = L == Loop::xyd_pair2 || L == Loop::xyd_x2 ? 2 : (L == Loop::xyd_x4 ? 4 : 1);
        const bool fast = MAP == MGDP_MAP_CELL && geo.HW <= CPT * (int)blockDim.x;
        const bool soa = SOA_ONLY || (fast && !geo.pair && !geo.quad);
        if (!SERVED) copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
        if (!soa) {
            // cell-major paths use the first S entries of each (Ss-sized) tile
            if (k == 0) zero16(V0, geo.S * (int)sizeof(T));
            else copy16(V0, V + vb, geo.S * (int)sizeof(T));
        }
        // the served pair loop's fresh start needs no stage here: it clears its flag bytes once per grid and
        // sets its first pair's in its own first stage (fused_serve_pair)
        bool own_start = false;
        if constexpr (L == Loop::serve_pair) own_start = sc->ew != 0 && k == 0;
        if (!own_start) {
            if (threadIdx.x < 64) flags[threadIdx.x] = 0;
            __syncthreads();
        }
        // Irregular: a served solve is always own-rule, so Loop::wave and the one-thread-per-cell loops the
        // server also runs pick the own-rule instantiation by SERVED || own
        if constexpr (L == Loop::wave) {  // lone XYD grid on one wave, N cells per lane (host: B == 1, blockDim 64)
            static_assert(MODEL == MGDP_MODEL_XYD && MAP == MGDP_MAP_CELL, "one-wave path is XYD, cell mapping");
            MGDP_BY_RULE(SERVED || own,
                         fused_wave_xyd<T, SLIP, OWN_RULE, N>(geo, cf, cl, V0, V1, V + vb, V + vb, pi + vb, k, k_target, dvl, done));
        } else if constexpr (L == Loop::xyd_pair2) {
            static_assert(MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL, "pair path: plain XYD");
            MGDP_BY_RULE(own,
                         fused_pair_xyd<T, OWN_RULE, 128 * N>(geo, cf, cl, V0, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl, done));
        } else if constexpr (MODEL == MGDP_MODEL_DOORKEY && L == Loop::dk_half) {
            MGDP_BY_RULE(own,
                         fused_dk_half<T, OWN_RULE, 64 * N>(geo, cf, cl, V0, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl, done));
        } else if constexpr (MODEL == MGDP_MODEL_DOORKEY && L == Loop::dk_1t) {
            MGDP_BY_RULE(own,
                         fused_fast_dk_1t<T, OWN_RULE>(geo, cf, cl, V0, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl, done));
        } else if constexpr (loop_is_serve_ew(L)) {
            static_assert(SERVED && MODEL == MGDP_MODEL_XYD && !SLIP && MAP == MGDP_MAP_CELL, "served plain XYD grid");
            if (sc->ew != 0) {
                if constexpr (L == Loop::serve_pair) {
                    // a fresh request of a grid the depth form takes: read off the goal depth; past the form's
                    // limits (path 2) nothing has been published or stored and the request sweeps from V_0
                    int path = 0;
                    if (sc->depth.ok && k == 0)
                        path = fused_serve_depth<T>(geo, cf, V + vb, pi + vb, k, dvl, done, sc->topo, sc->depth, sc->depth_max,
                                                    sc->depth_ktol);
                    sc->path = path;
                    if (path != 1) {
                        const int te = serve_pair_tile_elems(geo.HWs, geo.W);  // a tile: [pad][HWs][pad] cells of 4 planes
                        fused_serve_pair<T>(geo, cf, V0, V0 + te, slots, flags, V + vb, V + vb, pi + vb, k, dvl, done, sc->topo,
                                            sc->sp, sc->ew == 2);
                    }
                } else {
                    fused_serve_xyd<T>(geo, cf, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k, dvl, done, sc->topo, sc->ew == 2);
                }
            } else {  // this grid's wave edges do not allow the served loop: the general one
                fused_fast_xyd_soa<T, false, true>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl, done,
                                                   nullptr, nullptr, 0, &sc->topo);
            }
        } else if constexpr (MODEL == MGDP_MODEL_XYD && CPT > 1) {
            MGDP_BY_RULE(own,
                         fused_fast_xyd_soa_xn<T, SLIP, OWN_RULE, CPT>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k, k_target,
                                                             dvl, done));
        } else if (SERVED || soa) {  // served lone grids are always on this path (serve_eligible)
            if constexpr (MODEL == MGDP_MODEL_XYD) {
                MGDP_BY_RULE(SERVED || own,
                             fused_fast_xyd_soa<T, SLIP, OWN_RULE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl,
                                                         done, nullptr, nullptr, 0, sc ? &sc->topo : nullptr));
            } else {
                // batched grids: the special-first thread -> cell map (dk_class_perm) in the unused pi region
                // (tried: thread t on cell t, DESIGN.md 11.2 -- slower)
                uint8_t *perm = (!SERVED && 2 * geo.HW + 16 + 128 <= LY.pi_bytes) ? reinterpret_cast<uint8_t *>(pis) : nullptr;
                MGDP_BY_RULE(SERVED || own,
                             fused_fast_dk_soa<T, OWN_RULE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k, k_target, dvl, done,
                                                  nullptr, nullptr, 0, sc ? &sc->topo : nullptr, perm));
            }
        } else if constexpr (!SERVED && !SOA_ONLY) {
            // The cell-major paths of Loop::generic (launches only): the pair and quad loops, else one
            // sweep_lds per iteration on two LDS tiles; V and pi leave through LDS.  (Tried as a function
            // of its own: one SGPR moved in the seven kernels that run it, so it stays in place.)
            int cur = 0;
            const T *Vfinal = nullptr;
            if (fast && MODEL == MGDP_MODEL_XYD && geo.pair) {
                int vf = 0;
                MGDP_BY_RULE(own, fused_fast_xyd2<T, SLIP, OWN_RULE>(geo, cf, cl, V0, pis, slots, flags, k, k_target, vf, dvl,
                                                                    done));
                Vfinal = V0 + vf * geo.S;
            } else if (MODEL == MGDP_MODEL_XYD && MAP == MGDP_MAP_CELL && geo.quad && 4 * geo.HW <= (int)blockDim.x) {
                MGDP_BY_RULE(own, fused_quad_xyd<T, SLIP, OWN_RULE>(geo, cf, cl, V0, V1, pis, slots, flags, k, k_target, cur,
                                                                   dvl, done));
            } else {
                int parity = 0;
                T diff = (T)0;
                while (true) {
                    const T *Vin = cur ? V1 : V0;
                    T *Vout = cur ? V0 : V1;
                    diff = sweep_lds<T, MODEL, SLIP, MAP, true, MAP == MGDP_MAP_SA>(geo, cf, cl, Vin, Vout, pis);
                    cur ^= 1;
                    ++k;
                    if (own) {
                        const bool more = block_any(diff >= cf.tol, flags, parity);
                        parity ^= 1;
                        if (!more || k >= geo.max_sweeps) break;
                    } else {
                        __syncthreads();
                        if (k >= k_target) break;
                    }
                }
                dvl = (double)block_max(diff, slots, 0);
                done(k, dvl);
                if (MAP == MGDP_MAP_CELL) {  // pi of the last sweep = argmax on V_{k-1}
                    sweep_lds<T, MODEL, SLIP, MAP, false, true>(geo, cf, cl, cur ? V0 : V1, nullptr, pis);
                    __syncthreads();
                }
            }
            copy16(V + vb, Vfinal ? Vfinal : (cur ? V1 : V0), geo.S * (int)sizeof(T));
            copy_pi(pi + vb, pis, geo.S);
        }
    }
    record_grid(geo, kenv, dvenv, e, k, dvl, writer());
    return true;
}
#undef MGDP_BY_RULE

// Loop::wave: the one-wave lone-grid variant (fused_wave_xyd), 64 threads, so its N cells per lane
// may use the whole register file.
template <typename T, int MODEL, bool SLIP, int MAP, Loop L = Loop::generic, int N = 0>
__global__ void __launch_bounds__(L == Loop::wave || L == Loop::wave2 || L == Loop::band ? 64 : (L == Loop::wave2n || L == Loop::mix ? 128 : 1024), wave2_min_waves<T>(L, N))
vi_fused_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V,
                int8_t *__restrict__ pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
                unsigned long long *__restrict__ host_out, int k_target, int fresh, int in_kernel_reduce,
                unsigned int epoch, const long long *__restrict__ k_target_dev,
                unsigned long long *__restrict__ host_mirror, unsigned long long *__restrict__ gk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem LY = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), geo.nbuf);
    constexpr bool kOwnLds = L == Loop::wave2 || L == Loop::wave2n || L == Loop::band || L == Loop::mix;  // wave2-family layouts, gk
    T *slots = reinterpret_cast<T *>(smem + (kOwnLds || loop_is_dkrow(L) ? 0 : LY.slots_off()));
    // a one-wave grid of a mixed launch: its second wave leaves before touching anything
    if constexpr (L == Loop::mix)
        if (threadIdx.x >= 64 && (int)blockIdx.x >= geo.nmix) return;
    // multi-GPU protocol (mgdp_vi_run_to_dev): the target sweep is the all-reduced K in device
    // memory, written by a collective ordered before this launch on the stream
    if (k_target_dev) {
        k_target = (int)k_target_dev[0];
        // mgdp_vi_run_to_dev_sync: the all-reduced word after K (the own-rule dV) goes to the host
        // with this launch's result, as two words tagged with this launch's epoch (the host waits
        // for them as for the result's)
        if (host_mirror && blockIdx.x == 0 && threadIdx.x == 0)
            publish_word2(host_mirror, (unsigned long long)k_target_dev[1], epoch);
    }
    int k;
    double dvl;
    // Loop::dk_rows: the wave index in an SGPR, for late_tid after the sweep loop (fused_dk_rows)
    const int wvk = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const bool lone = in_kernel_reduce && gridDim.x == 1;
    const bool work = fused_grid<T, MODEL, SLIP, MAP, false, L, N>(geo, cf, cells, V, pi, kenv, dvenv, host_out, k_target,
                                                                 fresh, lone, epoch,
                                                                 geo.order ? (int)geo.order[blockIdx.x] : (int)blockIdx.x,
                                                                 k, dvl, kOwnLds ? gk : nullptr);
    // a launch-wide-rule launch (wave2 with gk) reduces and publishes through its own counter tree
    const bool gk_pub = kOwnLds && gk != nullptr && k_target < 0 && !k_target_dev;
    if (in_kernel_reduce && !gk_pub)
        fused_reduce(red, ticket, host_out, k, dvl, reinterpret_cast<unsigned int *>(slots + 16), epoch, work,
                     loop_is_dkrow(L) ? late_tid(wvk) : (int)threadIdx.x);
}

// Persistent solver for a lone grid: one workgroup stays resident and serves solve requests posted
// in host-mapped memory, removing the launch and dispatch latency from every solve.  The grid is
// staged in LDS (and its topology resolved) at launch and again whenever a request carries
// kServeNewCells: the request's source word (host_cmd[1], tagged with the request's low 16 bits, so
// a source written before the request can never be paired with an older one) names the new grid's
// W*H bytes -- host-mapped staging or device memory --, which the workgroup reads with
// system-scope loads (coherent with the host and with every XCD's L2), copies into LDS and into
// the handle's HBM cells (so a later non-served launch sees the same grid).  Lane 0 of every
// polling wave reads the request word (relaxed system-scope loads, the waves staggered by s_sleep)
// and also watches the LDS word another wave may already have set.  By default only wave 0 polls
// (`pollers` = 1; the others wait at the barrier): with four staggered pollers the barrier also
// waited for the other waves' in-flight PCIe reads (measured 0.2-0.4 us per solve slower).
// poll_dma (default): the poller does not wait for its reads.  Each poll is an LDS-DMA load
// (global_load_lds_dwordx4 of the request / source pair) into a 16-B LDS mailbox, issued about
// every 60 ns, so a PCIe round trip's worth of polls is in flight and the mailbox always holds the
// latest read to return: a request is seen one round trip after it lands instead of one to two
// (one blocking read at a time put a 1.2-1.5 us sawtooth on the solve latency, by when the host
// posted relative to the poll -- tools/probe_serve.cpp with MGDP_PROBE_GAP_US).  The loads are
// asm the compiler does not track: a stray one still in flight when the request is seen writes only
// the mailbox, and the wave's next vmcnt wait (the compiler's, for its own accesses, or the one
// before the exit word) also covers it.  Request
// r (!= the last served) runs a fresh fused solve whose {k, dV} is published tagged with r.  Every
// wave leaves on the quit word, after `idle_ticks` without a request or after `life_ticks` in total
// (s_memrealtime, 100 MHz); the host relaunches the server if a request finds it gone.
constexpr int kHoutWords = 32;  // host-mapped words of a handle (mgdp_vi::h_out)
constexpr int kHoutReq = 16;    // request word; its source word follows (one 16-B pair)
constexpr int kHoutPath = 28;   // Loop::serve_pair: the last request's path, then this launch's requests by path [3]
constexpr int kHoutClk = 24;    // a departing server's {shader-clock cycles, 100 MHz ticks} of its life,
                                // then {100 MHz ticks inside its solves, solves served}
constexpr unsigned long long kServeQuit = ~0ull;
constexpr unsigned long long kServeNewCells = 1ull << 62;
constexpr unsigned long long kServeLast = 1ull << 61;  // request flag: leave after serving it
constexpr unsigned long long kServeSrcMask = (1ull << 48) - 1;

// One poll of the {request, source} pair (16 B of host memory, system scope) into the LDS mailbox
// `box` by LDS DMA, issued by the calling lane without waiting for it (see vi_serve_kernel).  At
// most 24 stay in flight (about 1.5 us of polls at the loop's pace; the wait is free below that).
// M0 holds the LDS address for the load and is restored after it.
__device__ __forceinline__ void poll_issue(const unsigned long long *src, unsigned long long *box) {
    const unsigned int lds = (unsigned int)(uintptr_t)box;  // low 32 bits of a shared pointer: its LDS offset
    unsigned int m0_saved;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off sc0 sc1\n\t"
        "s_nop 0\n\t"
        "s_mov_b32 m0, %0\n\t"
        "s_waitcnt vmcnt(24)"
        : "=&s"(m0_saved)
        : "s"(lds), "v"(src)
        : "memory");
}

// (Loop::serve_pair: <= 4 waves by the plan's serve_ew rule, so its three register sets and halo state may
// use up to 512 VGPRs per lane: no spill)
template <typename T, int MODEL, bool SLIP, int MAP, Loop L = Loop::generic, int N = 0>
__global__ void __launch_bounds__(L == Loop::wave ? 64 : (L == Loop::serve_pair ? 256 : 1024))
vi_serve_kernel(Geo geo, Coef<T> cf, uint8_t *__restrict__ cells, T *__restrict__ V,
                int8_t *__restrict__ pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                unsigned long long *__restrict__ host_out, const unsigned long long *__restrict__ host_cmd,
                unsigned long long served, unsigned long long idle_ticks, unsigned long long life_ticks, int pollers,
                unsigned long long exit_tag, int poll_dma, int depth_max) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long s_cmd, s_src;
    __shared__ __attribute__((aligned(16))) unsigned long long s_box[2];  // poll mailbox: {request, source}
    const Smem LY = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), geo.nbuf);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + LY.cells_off());
    copy16(cl, cells, geo.HWp);
    if (threadIdx.x == 0) {
        s_cmd = served;
        s_box[0] = served;
        s_box[1] = 0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c_start = __builtin_amdgcn_s_memtime();  // shader-clock cycles
    unsigned long long t_last = t_start;
    // GPU-side time of the solves (thread 0: the poll that saw the request -> the solve's end,
    // s_memrealtime ticks already read for the idle limit, so no extra counter read per solve)
    unsigned long long t_seen = t_start, busy = 0, solves = 0;
    // the depth form's table of this launch (gamma, tol and the dtype are the handle's): vi_serve_depth.h
    if constexpr (L == Loop::serve_pair && MODEL == MGDP_MODEL_XYD)
        if (depth_max > 0) serve_depth_table<T>(cf);
    __syncthreads();
    // the grid stays put between kServeNewCells requests: resolve this thread's cell topology once
    ServeCtx<T, MODEL> sc = {};
    unsigned long long n_path[3] = {0, 0, 0};  // thread 0: this launch's requests by path (Loop::serve_pair)
    int last_path = 0;
    if constexpr (L == Loop::serve_pair && MODEL == MGDP_MODEL_XYD) {
        sc.depth_max = depth_max;
        sc.depth_ktol = depth_max > 0 ? serve_depth_ktol() : 0;
    }
    __shared__ int s_ew;
    auto resolve = [&]() {
        if constexpr (L == Loop::generic || loop_is_serve_ew(L)) {
            const int cc = (int)threadIdx.x < geo.HW ? (int)threadIdx.x : 0;
            if constexpr (MODEL == MGDP_MODEL_XYD) sc.topo = xyd_topo_soa<T>(cl, geo, cc);
            else sc.topo = dk_topo_soa(cl, geo, cc);
        }
        if constexpr (L == Loop::serve_pair && MODEL == MGDP_MODEL_XYD) sc.sp = serve_pair_topo<T>(cl, geo, cf, sc.topo, (int)threadIdx.x);
        if constexpr (loop_is_serve_ew(L)) sc.ew = serve_ew_ok(cl, geo, &s_ew) ? 2 : 0;
        if constexpr (L == Loop::serve_pair && MODEL == MGDP_MODEL_XYD)
            sc.depth = serve_depth_topo(cl, geo, depth_max > 0 && sc.ew != 0);
    };
    resolve();
    while (true) {
        if (lane == 0 && wave < pollers) {  // the other waves wait at the barrier
            for (int i = 0; i < wave; ++i) __builtin_amdgcn_s_sleep(8);  // stagger the pollers
            while (true) {
                unsigned long long cmd, src = 0;
                if (poll_dma) {
                    poll_issue(host_cmd, s_box);
                    __builtin_amdgcn_s_sleep(1);
                    cmd = __hip_atomic_load(&s_box[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    src = __hip_atomic_load(&s_box[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    cmd = __hip_atomic_load(host_cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                if (cmd != served) {
                    t_seen = now;
                    if (cmd != kServeQuit && (cmd & kServeNewCells)) {
                        // the host wrote the source word before the request word; its tag proves it
                        // belongs to this request (a stale read is simply repeated)
                        if (!poll_dma || (src >> 48) != (cmd & 0xffffull))
                            src = __hip_atomic_load(host_cmd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        while ((src >> 48) != (cmd & 0xffffull)) {
                            if (__builtin_amdgcn_s_memrealtime() - t_start > life_ticks) { cmd = kServeQuit; break; }
                            src = __hip_atomic_load(host_cmd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                        __hip_atomic_store(&s_src, src & kServeSrcMask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    __hip_atomic_store(&s_cmd, cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                if (__hip_atomic_load(&s_cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != served) break;
                if (now - t_last > idle_ticks || now - t_start > life_ticks) {
                    __hip_atomic_store(&s_cmd, kServeQuit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                if (!poll_dma) __builtin_amdgcn_s_sleep(2);
            }
        }
        __syncthreads();
        const unsigned long long cmd = s_cmd;
        if (cmd == kServeQuit) break;
#ifdef MGDP_SERVE_TRACE
        if (threadIdx.x == 0) {  // s_memtime counts shader-clock cycles, s_memrealtime 100 MHz ticks
            __hip_atomic_store(host_out + 14, __builtin_amdgcn_s_memtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_out + 8, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
#endif
        if (cmd & kServeNewCells) {  // restage the grid named by the request
            const uint8_t *src = reinterpret_cast<const uint8_t *>(s_src);
            for (int i = threadIdx.x; i < geo.HW; i += blockDim.x) {
                const uint8_t b = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                cl[i] = b;
                cells[i] = b;
            }
            __syncthreads();
            resolve();
        }
        int k;
        double dvl;
        sc.path = 0;
        if (!fused_grid<T, MODEL, SLIP, MAP, true, L, N>(geo, cf, cells, V, pi, kenv, dvenv, host_out, -1, 1, true,
                                                   (unsigned int)cmd, 0, k, dvl, nullptr, &sc) &&
            threadIdx.x == 0)
            publish_tagged(host_out, k, dvl, (unsigned int)cmd);
        if constexpr (L == Loop::serve_pair) {
            // the path this request took, counted in registers: the words leave with the server's exit words
            // (mgdp_vi_serve_path reads them once it has left), so a request pays no host store for them
            if (threadIdx.x == 0) {
                last_path = sc.path;
                if (sc.path == 0) ++n_path[0];  // (no indexed access: the counters stay in registers)
                else if (sc.path == 1) ++n_path[1];
                else ++n_path[2];
#ifdef MGDP_SERVE_TRACE
                if (sc.path == 1)  // the depth form's "V and pi stores issued" stamp (vi_serve_depth.h)
                    __hip_atomic_store(host_out + 10, g_pair_trace[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
            }
            // a depth-form solve leaves the tiles alone: their once-per-grid clear is still to come
            if (sc.ew == 2 && sc.path != 1) sc.ew = 1;  // the tiles' pads stay +0 until the next grid
        } else if (sc.ew == 2) {
            sc.ew = 1;
        }
        served = cmd;
        t_last = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            busy += t_last - t_seen;
            ++solves;
        }
        if (cmd & kServeLast) break;
        // Every wave is past s_cmd and the LDS tiles before the next request: an LDS-only barrier.
        // The V / pi stores of this solve stay in flight while the next request is polled (a
        // __syncthreads would drain them first); the host reads V / pi only after server_stop
        // has drained the stream.
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // Leaving: every wave's V / pi stores complete, then one system-scope release tells the host
    // (server_stop without a drain waits for this word instead of the stream's completion signal).
    // The word is this launch's own tag, so an earlier server's late exit store can never satisfy
    // the wait for a later one.
    // The launch's shader-clock cycles and 100 MHz ticks go out with it (kHoutClk): the host turns
    // them into the clock the server ran at (mgdp_vi_serve_clock), at no cost per solve.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(host_out + kHoutClk, __builtin_amdgcn_s_memtime() - c_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 1, __builtin_amdgcn_s_memrealtime() - t_start, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 2, busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 3, solves, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if constexpr (L == Loop::serve_pair) {
            if (solves > 0) {  // the last request's path and this launch's requests by path
                __hip_atomic_store(host_out + kHoutPath, (unsigned long long)last_path, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                for (int i = 0; i < 3; ++i)
                    __hip_atomic_store(host_out + kHoutPath + 1 + i, n_path[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        __hip_atomic_store(host_out + 11, exit_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Persistent server for a resident batch (round 6): the resident one-wave batch (fused_wave2_xyd,
// B <= the kernel's resident capacity, deterministic XYD grids) stays on the device between
// solves, so a solve costs a request word instead of a launch, a dispatch of B workgroups, their
// cells copy and the end-of-kernel release.  Every request is a full solve from
// V_0 = 0 with the in-launch reduction (GkCtx) publishing {kmax, dV, kmin} tagged with the request
// exactly as a launch does; nothing is carried from one request to the next but the grids' cells
// in LDS.  Lane 0 of workgroup 0 (the forwarder) polls the host's request word (LDS-DMA mailbox,
// as vi_serve_kernel) and forwards it to `copies` device words, one per 128-B line (tag of this launch in bits
// 32..47, the request's epoch in the low 32 bits, kServeLast kept, kBreqQuit to leave); every
// other wave polls that word at agent scope with s_sleep between polls and at priority 0 (the
// waves still sweeping get the issue slots).  Only the forwarder decides to leave (quit word,
// idle or life limit); the others leave on its quit word, or after the life limit plus a grace
// period, so every wave reaches the exit.  The last wave out (a two-level exit counter) writes the exit
// word, as a lone server does.
constexpr unsigned long long kBreqQuit = 1ull << 63;
constexpr int kBreqExit = kBreqCopies * 16;                           // exit counters: 64 shard lines, then the top line
constexpr int kBreqExitShards = 64;
constexpr int kBreqWords = kBreqExit + (kBreqExitShards + 1) * 16;
constexpr unsigned long long kBserveGraceTicks = 100000000ull;        // 1 s at 100 MHz
__device__ __forceinline__ unsigned long long rfl64(unsigned long long x) {
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)x);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// Waves per SIMD the server is compiled for: those of the fused kernel's wave2 instantiation of the
// same P (its resident capacity; fp32 P = 3: 5 instead of 7, which spilled).  Inside the request loop
// the compiler spent 25-60 % more VGPRs on the same sweep loop (fp32 P = 6: 173 vs 115 -- half the
// grids resident); with the lane index opaque per request (fused_wave2_xyd OPQ) and this bound,
// every instantiation fits without scratch.
template <typename T>
__host__ __device__ constexpr int bserve_min_waves(int P) {
    return sizeof(T) == 4 ? (P <= 2 ? 8 : P <= 4 ? 5 : P <= 6 ? 4 : 3)
                          : (P == 1 ? 8 : P == 2 ? 5 : P == 3 ? 4 : P == 4 ? 3 : P <= 7 ? 2 : 1);
}
// MULTI: the launch has fewer workgroups than grids (a batch past the resident capacity, MGDP_BSERVE=2):
// its own instantiation, so the resident loop keeps its registers.
template <typename T, int P, bool MULTI = false>
__global__ void __launch_bounds__(64, bserve_min_waves<T>(P))
vi_bserve_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V,
                 int8_t *__restrict__ pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                 unsigned long long *__restrict__ host_out, const unsigned long long *__restrict__ host_cmd,
                 unsigned long long *__restrict__ breq, unsigned long long *__restrict__ gk, unsigned long long served,
                 unsigned long long idle_ticks, unsigned long long life_ticks, unsigned long long exit_tag, int copies,
                 int nap, int wait_pub, int prio_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ __attribute__((aligned(16))) unsigned long long s_box[2];  // the forwarder's poll mailbox
    const int lane = (int)threadIdx.x;
    constexpr bool multi = MULTI;  // past the resident capacity: several grids per workgroup
    const int e = multi ? 0 : (geo.order ? (int)geo.order[blockIdx.x] : (int)blockIdx.x);
    uint8_t *cl = smem + 256;
    if (!multi) copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
    T *tile = reinterpret_cast<T *>(smem + wave2_tile_off(geo.HWp));
    const bool fwd = blockIdx.x == 0;
    const unsigned long long tg = (exit_tag & 0xffffull) << 32;
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c_start = __builtin_amdgcn_s_memtime();
    unsigned long long t_last = t_start, busy = 0, solves = 0;
    if (fwd && lane == 0) {
        s_box[0] = served;
        s_box[1] = 0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: its LDS accesses are in order
    const long long vb = (long long)e * geo.S;
    while (true) {
        unsigned long long cmd;
        __builtin_amdgcn_s_setprio(0);  // polling: the waves still sweeping get the issue slots
        if (fwd) {
            unsigned long long c = served;
            // Host polls are PCIe reads the forwarder keeps in flight (up to 24, LDS DMA); while other grids
            // of the request still sweep they would hold its CU's memory path (trace build: the grids
            // that finished 15-18 us after the rest).  So first wait, at agent scope, for the request's
            // publication (gk_exit's device copy of the epoch); the host posts the next one only after it.
            if (wait_pub && solves > 0) {
                while (__hip_atomic_load(gk + kGkTop2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
                       (served & 0xffffffffull)) {
                    if (__builtin_amdgcn_s_memrealtime() - t_start > life_ticks) break;
                    __builtin_amdgcn_s_sleep(4);
                }
                t_last = __builtin_amdgcn_s_memrealtime();  // the idle limit counts from the publication
            }
            if (lane == 0) {
                while (true) {
                    poll_issue(host_cmd, s_box);
                    __builtin_amdgcn_s_sleep(1);
                    c = __hip_atomic_load(&s_box[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (c != served) break;
                    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                    if (now - t_last > idle_ticks || now - t_start > life_ticks) {
                        c = kServeQuit;
                        break;
                    }
                }
            }
            cmd = rfl64(c);
            const unsigned long long dw =
                cmd == kServeQuit ? (tg | kBreqQuit) : (tg | (cmd & 0xffffffffull) | (cmd & kServeLast));
            if (lane < copies) {
#ifdef MGDP_BSERVE_TRACE  // trace build: the forwarder's request-seen stamp beside each copy
                __hip_atomic_store(breq + lane * 16 + 1, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#endif
                __hip_atomic_store(breq + lane * 16, dw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            unsigned long long dw;
            const unsigned long long *word = breq + (blockIdx.x % (unsigned)copies) * 16u;
            while (true) {  // the whole wave loads the word (one request): no divergent loop
                dw = rfl64(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if ((dw & (0xffffull << 32)) == tg &&
                    ((dw & kBreqQuit) || (dw & 0xffffffffull) != (served & 0xffffffffull)))
                    break;
                if (__builtin_amdgcn_s_memrealtime() - t_start > life_ticks + kBserveGraceTicks) {
                    dw = tg | kBreqQuit;
                    break;
                }
                for (int i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(10);
            }
            cmd = (dw & kBreqQuit) ? kServeQuit : ((dw & 0xffffffffull) | (dw & kServeLast));
        }
        if (cmd == kServeQuit) break;
        // the first prio_n workgroups hold the dispatch order's longest grids (MGDP_BSERVE_PRIO_FRAC)
        if ((int)blockIdx.x < prio_n) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
        const unsigned long long t_seen = __builtin_amdgcn_s_memrealtime();
        int k = 0;
        double dvl = 0.0;
        auto done = [](int, double) {};
        if constexpr (MULTI) {
            // More grids than workgroups: this workgroup solves the dispatch order's positions
            // blockIdx.x, + G, + 2G, ... (round-robin over the longest-first order), each from V_0 = 0
            // with its cells staged in turn, and arrives ONCE at the counter tree with its grids'
            // {min, max} sweeps and max dV (a per-grid arrival would hold the wave on its ticket's round
            // trip before every next grid).
            int kmn = 0x7fffffff, kmx = 0;
            double dvm = 0.0;
            for (int i = (int)blockIdx.x; i < geo.B; i += (int)gridDim.x) {
                const int eg = geo.order ? (int)geo.order[i] : i;
                const long long vg = (long long)eg * geo.S;
                copy16(cl, cells + (long long)eg * geo.HWp, geo.HWp);
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // one wave: the cells are in place
                int kg = 0;
                double dg = 0.0;
                fused_wave2_xyd<T, true, P, true, true>(geo, cf, cl, tile, V + vg, V + vg, pi + vg, kg, -1, dg, done,
                                                        GkCtx{});
                record_grid(geo, kenv, dvenv, eg, kg, dg, lane == 0);
                kmn = min(kmn, kg);
                kmx = max(kmx, kg);
                dvm = dg > dvm ? dg : dvm;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            gk_exit<true>(GkCtx{gk, (unsigned int)cmd, (int)blockIdx.x, (int)gridDim.x, host_out}, kmx, dvm,
                          late_tid(0), kmn);
            k = kmx;
        } else {
            fused_wave2_xyd<T, true, P, true, true>(geo, cf, cl, tile, V + vb, V + vb, pi + vb, k, -1, dvl, done,
                                                    GkCtx{gk, (unsigned int)cmd, e, geo.B, host_out});
        }
        record_grid(geo, kenv, dvenv, e, k, dvl, lane == 0 && !multi);
#ifdef MGDP_BSERVE_TRACE  // trace build: this grid's start / end after the forwarder saw the request,
                          // 10 ns ticks in the low / high 16 bits of its executed-sweeps word
        if (lane == 0 && !multi) {
            const unsigned long long t0 = __hip_atomic_load(breq + (blockIdx.x % (unsigned)copies) * 16u + 1,
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
            const unsigned long long a = t_seen - t0 < 0xffffull ? t_seen - t0 : 0xffffull;
            const unsigned long long b = t1 - t0 < 0xffffull ? t1 - t0 : 0xffffull;
            if (geo.kexec) geo.kexec[e] = (int)(a | (b << 16));
        }
#endif
        served = cmd;
        t_last = __builtin_amdgcn_s_memrealtime();
        busy += t_last - t_seen;
        ++solves;
        if (cmd & kServeLast) break;
    }
    // Leaving: this wave's stores complete (the exit V / pi stores are write-through, the clock words
    // system-scope: drained means written), then the exit counters; the last wave out resets them and
    // writes the launch's exit word.  Waves leaving after a kServeLast request do it while that
    // request's long grids still sweep, so (tools/probe_bserve.py, the last request's wall): no wave
    // but the last fences (a system-scope release writes back the L2: +35-60 us), and the count is a
    // two-level tree like the solve's (64 shard lines, then a top line) -- 8192 atomics on one word
    // serialised at ~10 ns each ahead of the request's own publication: +82 us.
    if (lane == 0 && fwd) {
        __hip_atomic_store(host_out + kHoutClk, __builtin_amdgcn_s_memtime() - c_start, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 1, __builtin_amdgcn_s_memrealtime() - t_start, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 2, busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_out + kHoutClk + 3, solves, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        const unsigned int G = gridDim.x;
        const unsigned int nsh = G < (unsigned)kBreqExitShards ? G : (unsigned)kBreqExitShards;
        const unsigned int sh = blockIdx.x % nsh;
        const unsigned long long size = G / nsh + (sh < G % nsh ? 1u : 0u);
        unsigned long long *cnt = breq + kBreqExit + sh * 16u, *top = breq + kBreqExit + kBreqExitShards * 16;
        if (__hip_atomic_fetch_add(cnt, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == size - 1ull) {
            __hip_atomic_store(cnt, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (__hip_atomic_fetch_add(top, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsh - 1ull) {
                __hip_atomic_store(top, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(host_out + 11, exit_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// The fused solve with the SURVEY 8(f) item-3 options (ND = NoDeath lava, HMODE = finite horizon
// 1 / with pi_t 2): one workgroup per grid on the direction-major one-thread-per-cell path only
// (the host enforces MGDP_MAP_CELL and no pair / quad steps when options are set).
template <typename T, int MODEL, bool SLIP, bool ND, int HMODE>
__global__ void __launch_bounds__(1024)
vi_fused_opts_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V,
                     int8_t *__restrict__ pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                     unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
                     unsigned long long *__restrict__ host_out, int k_target, int fresh, int in_kernel_reduce,
                     unsigned int epoch, const T *__restrict__ rgoal, int8_t *__restrict__ pi_t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem L = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), geo.nbuf);
    T *V0 = reinterpret_cast<T *>(smem);
    T *V1 = reinterpret_cast<T *>(smem + L.v_bytes);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + L.cells_off());
    T *slots = reinterpret_cast<T *>(smem + L.slots_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + L.flags_off());
    const int e = blockIdx.x;
    int k = fresh ? 0 : kenv[e];
    double dvl = fresh ? 0.0 : dvenv[e];
    // fixed-point completion; not for a finite horizon, whose sweeps depend on the step
    if (HMODE == 0 && grid_complete_at(k, dvl, k_target)) {
        if (threadIdx.x == 0) kenv[e] = k_target;
        k = k_target;
    }
    const bool work = grid_has_work(geo, k, dvl, k_target);
    const bool lone = in_kernel_reduce && gridDim.x == 1;
    if (work) {
        const long long vb = (long long)e * geo.S;
        copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
        if (threadIdx.x < 64) flags[threadIdx.x] = 0;
        __syncthreads();
        auto done = [&](int kk, double dv) { publish_solve<false>(host_out, kk, dv, epoch, lone, threadIdx.x == 0); };
        int8_t *pit = HMODE == 2 ? pi_t + vb : nullptr;
        const long long pstride = (long long)geo.B * geo.S;
        if constexpr (MODEL == MGDP_MODEL_XYD) {
            if constexpr (HMODE == 0) {
                if (k_target < 0)
                    fused_fast_xyd_soa<T, SLIP, true, ND, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb,
                                                                 k, k_target, dvl, done, rgoal, pit, pstride);
                else
                    fused_fast_xyd_soa<T, SLIP, false, ND, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb,
                                                                  k, k_target, dvl, done, rgoal, pit, pstride);
            } else {  // finite horizon: exactly k_target = H sweeps
                fused_fast_xyd_soa<T, SLIP, false, ND, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb,
                                                              k, k_target, dvl, done, rgoal, pit, pstride);
            }
        } else {
            if constexpr (HMODE == 0) {
                if (k_target < 0)
                    fused_fast_dk_soa<T, true, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k,
                                                      k_target, dvl, done, rgoal, pit, pstride);
                else
                    fused_fast_dk_soa<T, false, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k,
                                                       k_target, dvl, done, rgoal, pit, pstride);
            } else {
                fused_fast_dk_soa<T, false, HMODE>(geo, cf, cl, V0, V1, slots, flags, V + vb, V + vb, pi + vb, k,
                                                   k_target, dvl, done, rgoal, pit, pstride);
            }
        }
        record_grid(geo, kenv, dvenv, e, k, dvl, threadIdx.x == 0);
    }
    if (in_kernel_reduce)
        fused_reduce(red, ticket, host_out, k, dvl, reinterpret_cast<unsigned int *>(slots + 16), epoch, work,
                     (int)threadIdx.x);
}

// Dispatch order from the cells (round 6): a proxy for the sweep at which each grid's own rule stops,
// computed once per cells load, so the longest grids start first from a handle's FIRST solve on.
// For a deterministic grid that stop is the longest shortest path to the goal (plus one sweep), so the
// proxy is a breadth-first depth over cells (moves only, no turns): XYD, the farthest walkable cell
// from a goal; DoorKey, the larger of that (doors and keys passable) and the farthest cell of the
// key's side (door shut) from the key plus the key's distance to the goal (fetch the key, then the
// goal).  Spearman rank correlation with the own-rule stopping sweep over reference-generated grids
// (orc_vi_fp): FourRooms 0.985, LavaS11N5 0.873, DoorKey-16 0.994.  Results never
// depend on it.  One 64-lane workgroup per grid, level-synchronous BFS in LDS (a lane's LDS accesses
// are ordered and a cell at level L+1 is only set next to one at level L, so no barrier is needed).
constexpr int kDepthMaxHW = 1024;
__device__ __forceinline__ int depth_bfs(const uint8_t *cl, uint16_t *dist, int HW, int W, int src_type,
                                         bool dk_open) {
    const int lane = threadIdx.x;
    constexpr uint16_t kUnseen = 0xffff;
    auto passable = [&](int t) { return dk_open ? (xyd_free(t) || t == T_DOOR || t == T_KEY) : xyd_free(t); };
    for (int c = lane; c < HW; c += 64) dist[c] = cl[c] == src_type ? 0 : kUnseen;
    int level = 0, maxd = 0;
    while (true) {
        bool grew = false;
        for (int c = lane; c < HW; c += 64) {
            if (dist[c] != kUnseen || !passable(cl[c])) continue;
            const bool nb = (c >= W && dist[c - W] == level) || (c + W < HW && dist[c + W] == level) ||
                            (c % W != 0 && dist[c - 1] == level) || (c % W != W - 1 && dist[c + 1] == level);
            if (nb) {
                dist[c] = (uint16_t)(level + 1);
                grew = true;
            }
        }
        if (__ballot(grew) == 0ull) break;
        maxd = ++level;
    }
    return maxd;
}
__global__ void __launch_bounds__(64) vi_depth_kernel(Geo geo, const uint8_t *__restrict__ cells, int model,
                                                      int32_t *__restrict__ depth) {
    __shared__ uint8_t cl[kDepthMaxHW];
    __shared__ uint16_t d1[kDepthMaxHW], d2[kDepthMaxHW];
    const int b = blockIdx.x, HW = geo.HW, W = geo.W;
    for (int c = threadIdx.x; c < HW; c += 64) cl[c] = cells[(long long)b * geo.HWp + c];
    int proxy = depth_bfs(cl, d1, HW, W, T_GOAL, model == MGDP_MODEL_DOORKEY);
    if (model == MGDP_MODEL_DOORKEY) {
        // the key's distance to the goal (doors and keys passable: d1), then the key side's depth
        int kd = 0x7fffffff;
        for (int c = threadIdx.x; c < HW; c += 64)
            if (cl[c] == T_KEY && d1[c] != 0xffff) kd = min(kd, (int)d1[c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) kd = min(kd, __shfl_xor(kd, o));
        const int side = depth_bfs(cl, d2, HW, W, T_KEY, false);
        if (kd != 0x7fffffff) proxy = max(proxy, side + kd);
    }
    if (threadIdx.x == 0) depth[b] = proxy;
}

// The sharded protocol's gate (mgdp_vi_run_to_dev_sync): kdv = the all-reduced {K, E}, written by
// the collective ordered before this launch.  E == 0: every grid everywhere is at an exact fixed
// point, so the result is {K, dV 0, K}; else kmin = kGateMore asks the host for run_to(K).
constexpr unsigned long long kGateMore = 0xffffffffull;
__global__ void __launch_bounds__(64) vi_gate_kernel(const long long *__restrict__ kdv,
                                                     unsigned long long *__restrict__ host_out, unsigned int epoch) {
    if (threadIdx.x == 0) {
        const unsigned long long K = (unsigned long long)kdv[0], E = (unsigned long long)kdv[1];
        publish_word2(host_out + 12, E, epoch);  // six tagged words, no drain between them
        publish(host_out, K, 0ull, E == 0 ? K : kGateMore, epoch);
    }
}

// Large batches: one workgroup reduces the per-grid (kenv, dvenv) into host-mapped memory (a
// single arrival ticket shared by tens of thousands of workgroups would serialise on one address).
__global__ void __launch_bounds__(1024)
vi_reduce_kernel(const int32_t *__restrict__ kenv, const double *__restrict__ dvenv, int B,
                 unsigned long long *__restrict__ host_out, unsigned int epoch) {
    __shared__ unsigned long long sk[16], sd[16], sn[16];
    unsigned long long km = 0, dm = 0, kn = 0x7fffffffull;
    auto fold = [&](int k, double d) {
        km = max(km, (unsigned long long)k);
        kn = min(kn, (unsigned long long)k);
        dm = max(dm, (unsigned long long)__double_as_longlong(d));
    };
    // 16-B loads, U of them in flight per thread before any is folded: one workgroup streaming
    // 12 B per grid is latency-bound (the one-load-per-iteration loop took 24 us for 65536 grids)
    constexpr int U = 4;
    const int B4 = B / 4;  // kenv / dvenv come from hipMalloc: 16-B aligned
    const int4 *k4 = reinterpret_cast<const int4 *>(kenv);
    const double2 *d2 = reinterpret_cast<const double2 *>(dvenv);
    const int step = (int)blockDim.x;
    for (int base = threadIdx.x; base < B4; base += U * step) {
        int4 kk[U];
        double2 da[U], db[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(base + u * step, B4 - 1);  // clamped re-reads are harmless for max/min
            kk[u] = k4[i];
            da[u] = d2[2 * i];
            db[u] = d2[2 * i + 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            fold(kk[u].x, da[u].x);
            fold(kk[u].y, da[u].y);
            fold(kk[u].z, db[u].x);
            fold(kk[u].w, db[u].y);
        }
    }
    for (int i = 4 * B4 + (int)threadIdx.x; i < B; i += step) fold(kenv[i], dvenv[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        km = max(km, (unsigned long long)__shfl_xor(km, o));
        dm = max(dm, (unsigned long long)__shfl_xor(dm, o));
        kn = min(kn, (unsigned long long)__shfl_xor(kn, o));
    }
    if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = km; sd[threadIdx.x >> 6] = dm; sn[threadIdx.x >> 6] = kn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) { km = max(km, sk[i]); dm = max(dm, sd[i]); kn = min(kn, sn[i]); }
        publish(host_out, km, dm, kn, epoch);
    }
}

// The same reduction over kRedShards workgroups (one shard each, so no two workgroups share an
// atomic address), the last arrival folding the shards and publishing -- fused_reduce's protocol,
// whose shards and ticket are idle when the fused launch does not reduce (B > inkernel_max).
__global__ void __launch_bounds__(256)
vi_reduce_multi_kernel(const int32_t *__restrict__ kenv, const double *__restrict__ dvenv, int B,
                       unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
                       unsigned long long *__restrict__ host_out, unsigned int epoch) {
    __shared__ unsigned long long sk[4], sd[4], sn[4];
    __shared__ unsigned int last;
    unsigned long long km = 0, dm = 0, kn = 0x7fffffffull;
    auto fold = [&](int k, double d) {
        km = max(km, (unsigned long long)k);
        kn = min(kn, (unsigned long long)k);
        dm = max(dm, (unsigned long long)__double_as_longlong(d));
    };
    constexpr int U = 4;
    const int B4 = B / 4;
    const int4 *k4 = reinterpret_cast<const int4 *>(kenv);
    const double2 *d2 = reinterpret_cast<const double2 *>(dvenv);
    const int step = (int)(blockDim.x * gridDim.x);
    for (int base = (int)(blockIdx.x * blockDim.x + threadIdx.x); base < B4; base += U * step) {
        int4 kk[U];
        double2 da[U], db[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(base + u * step, B4 - 1);  // clamped re-reads are harmless for max/min
            kk[u] = k4[i];
            da[u] = d2[2 * i];
            db[u] = d2[2 * i + 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            fold(kk[u].x, da[u].x);
            fold(kk[u].y, da[u].y);
            fold(kk[u].z, db[u].x);
            fold(kk[u].w, db[u].y);
        }
    }
    if (blockIdx.x == 0)
        for (int i = 4 * B4 + (int)threadIdx.x; i < B; i += (int)blockDim.x) fold(kenv[i], dvenv[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        km = max(km, (unsigned long long)__shfl_xor(km, o));
        dm = max(dm, (unsigned long long)__shfl_xor(dm, o));
        kn = min(kn, (unsigned long long)__shfl_xor(kn, o));
    }
    if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = km; sd[threadIdx.x >> 6] = dm; sn[threadIdx.x >> 6] = kn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) { km = max(km, sk[i]); dm = max(dm, sd[i]); kn = min(kn, sn[i]); }
        unsigned long long *r = red + (blockIdx.x & (kRedShards - 1)) * 4;
        const unsigned long long a = __hip_atomic_fetch_max(r + 0, km, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_fetch_max(r + 1, dm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c = __hip_atomic_fetch_min(r + 2, kn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" :: "v"(a), "v"(b), "v"(c) : "memory");
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x < 64) {  // every shard's updates returned before its ticket add
        unsigned long long *r = red + threadIdx.x * 4;
        unsigned long long x = __hip_atomic_exchange(r + 0, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long y = __hip_atomic_exchange(r + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long z = __hip_atomic_exchange(r + 2, 0x7fffffffull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            x = max(x, (unsigned long long)__shfl_xor(x, o));
            y = max(y, (unsigned long long)__shfl_xor(y, o));
            z = min(z, (unsigned long long)__shfl_xor(z, o));
        }
        if (threadIdx.x == 0) {
            __hip_atomic_exchange(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            publish(host_out, x, y, z, epoch);
        }
    }
}

// Early exit of a speculatively enqueued sweep: the previous sweep already met the rule.
__device__ __forceinline__ bool prev_sweep_converged(const unsigned long long *shards, int k, double tol) {
    if (k <= 1) return false;
    const unsigned long long *prev = shards + (long long)(k - 2) * 8;
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmax(m, __longlong_as_double((long long)prev[i]));
    return m < tol;
}

// ------------------------------------------------------------------------------------------------
// One Jacobi sweep (index k, 1-based) of every grid, V double-buffered in HBM.  A workgroup
// stages a group of `m` consecutive grids (their V rows and cells are contiguous in HBM) into LDS
// with 16-B loads -- the LDS tile of the neighbourhood --, updates them from LDS and writes the
// new rows back with 16-B stores; m > 1 keeps more bytes in flight per load phase and amortises
// the barriers.  check_prev: skip when the previous sweep's global max|dV| was already < tol.
// POLICY: evaluate only, write pi.
// ------------------------------------------------------------------------------------------------
constexpr int kSweepBlock = 256;

template <typename T, int MODEL, bool SLIP, int MAP, bool POLICY>
__global__ void __launch_bounds__(kSweepBlock)
vi_sweep_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, const T *__restrict__ Vin,
                T *__restrict__ Vout, int8_t *__restrict__ pi, unsigned long long *__restrict__ shards,
                int k, int check_prev, int m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (check_prev && prev_sweep_converged(shards, k, geo.tol)) return;
    const int vbytes = geo.S * (int)sizeof(T), pib = (geo.S + 15) / 16 * 16;
    T *Vi = reinterpret_cast<T *>(smem);
    T *Vo = reinterpret_cast<T *>(smem + m * vbytes);
    int8_t *pis = reinterpret_cast<int8_t *>(smem + 2 * m * vbytes);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + 2 * m * vbytes + m * pib);
    T *slots = reinterpret_cast<T *>(smem + 2 * m * vbytes + m * pib + m * geo.HWp);
    const int ngroups = (geo.B + m - 1) / m;

    T acc = (T)0;
    for (int gidx = blockIdx.x; gidx < ngroups; gidx += gridDim.x) {
        const int e0 = gidx * m;
        const int me = min(m, geo.B - e0);
        const long long vb = (long long)e0 * geo.S;
        __syncthreads();  // the previous group's LDS tile is no longer read
        copy16(cl, cells + (long long)e0 * geo.HWp, me * geo.HWp);
        copy16_nt_in(Vi, Vin + vb, me * vbytes);
        __syncthreads();
        for (int j = 0; j < me; ++j)
            acc = vmax(acc, sweep_lds<T, MODEL, SLIP, MAP, !POLICY, POLICY || MAP == MGDP_MAP_SA>(
                                geo, cf, cl + j * geo.HWp, Vi + j * geo.S, Vo + j * geo.S, pis + j * pib));
        __syncthreads();
        if (!POLICY) {
            copy16_nt_out(Vout + vb, Vo, me * vbytes);
        } else {
            for (int j = 0; j < me; ++j) copy_pi(pi + vb + (long long)j * geo.S, pis + j * pib, geo.S);
        }
    }
    if (!POLICY) {
        const T bdv = block_max(acc, slots, 0);
        if (threadIdx.x == 0 && shards)
            atomicMax(shards + (long long)(k - 1) * 8 + (blockIdx.x & 7),
                      (unsigned long long)__double_as_longlong((double)bdv));
    }
}

// ------------------------------------------------------------------------------------------------
// Register-pipelined HBM sweep (one thread per cell, HW <= blockDim = HWs): a workgroup walks its
// grids e = blockIdx.x + i*gridDim.x.  Each thread loads its own cell's V row (16 B XYD, 64 B
// DoorKey fp32, coalesced) and a dword of cell bytes DEPTH grids ahead into registers, so the HBM
// reads of the next grids are in flight while the current one is computed and stored; at the top
// of an iteration the registers are written to the direction-major LDS tile (the neighbourhood
// the front-cell reads need, bank-conflict free), the thread keeps its own values in registers and
// stores its new row straight to HBM.  LDS is only the neighbour exchange: no output staging.
// Same backups and |dV| as vi_sweep_kernel (bit-identical); pi stays with vi_sweep_kernel<POLICY>.
// ------------------------------------------------------------------------------------------------
template <typename T, int MODEL>
struct PipeRow {
    static constexpr int NV = MODEL == MGDP_MODEL_XYD ? 1 : 4;  // V4 per cell
    V4<T> v[NV];
    uint32_t cw;  // cell bytes 4c .. 4c+3 (threads c < HWp/4)
};

// V is streamed once per sweep (Vin read, Vout written; the next sweep's Vin is the whole
// 553 MB array again, far past the 256 MB MALL), so the loads and stores are nontemporal:
// measured on empty16x65536 (profiles/r01_sweep_nt/): 107.8 µs plain, 101.5 µs stores only, 98.0 µs both.
template <typename T>
__device__ __forceinline__ void st_v4(V4<T> *dst, const V4<T> &v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(v.v[j], &dst->v[j]);
}
template <typename T>
__device__ __forceinline__ V4<T> ld_v4(const V4<T> *src) {
    V4<T> v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v.v[j] = __builtin_nontemporal_load(&src->v[j]);
    return v;
}

template <typename T, int MODEL, bool SLIP, int DEPTH>
__global__ void __launch_bounds__(1024)
vi_sweep_pipe_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, const T *__restrict__ Vin,
                     T *__restrict__ Vout, unsigned long long *__restrict__ shards, int k, int check_prev) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (check_prev && prev_sweep_converged(shards, k, geo.tol)) return;
    using Row = PipeRow<T, MODEL>;
    constexpr int NV = Row::NV;
    const int HWs = geo.HWs;
    T *Vt = reinterpret_cast<T *>(smem);
    uint8_t *cl = smem + (size_t)geo.Ss * sizeof(T);
    T *slots = reinterpret_cast<T *>(smem + (size_t)geo.Ss * sizeof(T) + geo.HWp);
    const int c = threadIdx.x;
    const bool own_cell = c < geo.HW;
    const bool cell_word = c < (geo.HWp >> 2);
    const int cc = own_cell ? c : 0;
    const int stride = gridDim.x;

    // Unconditional loads (clamped addresses: past the last grid, idle threads re-read a valid row
    // whose values are never used), so the loop body is straight-line and the compiler's vmcnt
    // waits count the DEPTH-1 younger fetches instead of draining them.
    const int cw_idx = cell_word ? c : 0;
    auto fetch = [&](int e, Row &r) {
        const long long ee = e < geo.B ? e : geo.B - 1;
        const V4<T> *src = reinterpret_cast<const V4<T> *>(Vin + ee * geo.S + (long long)cc * 4 * NV);
#pragma unroll
        for (int q = 0; q < NV; ++q) r.v[q] = ld_v4(src + q);
        r.cw = reinterpret_cast<const uint32_t *>(cells + ee * geo.HWp)[cw_idx];
    };
    Row rows[DEPTH];
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) fetch(blockIdx.x + s * stride, rows[s]);
    T acc = (T)0;
    auto step = [&](int e, Row &r) {
        // stage this grid's rows; every thread is past the previous grid's LDS reads (barrier below)
        if (MODEL == MGDP_MODEL_XYD) {
#pragma unroll
            for (int d = 0; d < 4; ++d) Vt[d * HWs + c] = r.v[0].v[d];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<V4<T> *>(Vt + (q * HWs + c) * 4) = r.v[q];
        }
        if (cell_word) reinterpret_cast<uint32_t *>(cl)[c] = r.cw;
        __syncthreads();
        // refill in place, DEPTH grids ahead: r is dead once staged (the thread's own values are read
        // back from the tile), so the loads need no register copies and stay in flight during this
        // grid's work
        fetch(e + DEPTH * stride, r);
        Row own;
        if (MODEL == MGDP_MODEL_XYD) {
#pragma unroll
            for (int d = 0; d < 4; ++d) own.v[0].v[d] = Vt[d * HWs + c];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) own.v[q] = *reinterpret_cast<const V4<T> *>(Vt + (q * HWs + c) * 4);
        }
        T *dst = Vout + (long long)e * geo.S + (long long)c * 4 * NV;
        if (MODEL == MGDP_MODEL_XYD) {
            const XydTopo<T> tp = xyd_topo_soa<T>(cl, geo, cc);
            T nbv[4];
            xyd_load_nb(tp, Vt, nbv);
            V4<T> out;
            uint32_t pk;
            const T dv = xyd_step<T, SLIP, false>(tp, cf, own.v[0], nbv, out, pk);
            if (own_cell) {
                st_v4(reinterpret_cast<V4<T> *>(dst), out);
                acc = vmax(acc, dv);
            }
        } else {
            const DkTopo tp = dk_topo_soa(cl, geo, cc);
            V4<T> nbs[4];
            dk_load_nb(tp, Vt, nbs);
            T in[16], outv[16];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) in[4 * q + j] = own.v[q].v[j];
            uint32_t pk[4];
            const T dv = dk_step<T, false>(tp, cf, in, nbs, outv, pk);
            if (own_cell) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    st_v4(reinterpret_cast<V4<T> *>(dst) + q, V4<T>{{outv[4 * q], outv[4 * q + 1], outv[4 * q + 2], outv[4 * q + 3]}});
                acc = vmax(acc, dv);
            }
        }
        __syncthreads();  // the tile is rewritten by the next grid
    };
    int e = blockIdx.x;
    bool more = true;
    while (more) {  // the register slots rotate: slot j holds the grid DEPTH strides ahead of it
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            if (e >= geo.B) { more = false; break; }
            step(e, rows[j]);
            e += stride;
        }
    }
    const T bdv = block_max(acc, slots, 0);
    if (threadIdx.x == 0 && shards)
        atomicMax(shards + (long long)(k - 1) * 8 + (blockIdx.x & 7), (unsigned long long)__double_as_longlong((double)bdv));
}

}  // namespace mgdp
