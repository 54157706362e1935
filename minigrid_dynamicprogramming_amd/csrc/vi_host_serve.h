// vi_host_serve.h -- the host's side of the solve protocol: reduce_env (the wait for a launch's or a
// server's published result), the eligibility predicates, the server's stop / exit wait / request /
// hand-off, the sweep method's sweep_run and shard_max, the sharded solve's comm_max_double, the state
// and preconditions the protocol entry points share, and the two halves of mgdp_vi_solve that are not a
// launch: solve_served (the resident-server request) and solve_close (the global rule of vi_rule.h on
// mgdp_vi_sweep, finish, report).  Part of the single translation unit vi.hip: included after
// vi_host_launch.h.
#pragma once

namespace {

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
    return vi->kn.persistent && vi->d_breq && vi->d_gk && !vi->timed.on && vi->d.B > 1 &&
           (vi->d.B <= vi->plan.bserve_cap || vi->plan.bserve_any) &&
           !vi->plan.opts && vi->d.method == MGDP_METHOD_FUSED && vi->d.horizon == 0 && vi->d.max_sweeps >= 1;
}
bool served_eligible(const mgdp_vi *vi) { return serve_eligible(vi) || bserve_eligible(vi); }
// Wait for the exit word of the latest server launch (its own tag: a late store of an earlier
// server cannot satisfy it); a server that never started or faulted is reported by the stream.
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
// Ask a resident server to leave and drain the stream.  Every entry point that enqueues other
// work on the stream, or reads results, calls this first.  A grid handed over for the next request
// but not yet served goes to d_cells here, so every other launch sees it.
// drain = false (mgdp_vi_synchronize): wait for the server's exit word -- its V / pi stores are
// then complete and visible, and nothing else is queued behind it -- instead of the stream's
// completion signal, which a later device synchronize still observes.
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
// ... and then whatever else the stream holds
int drain(mgdp_vi *vi) {
    if (int rc = server_stop(vi)) return rc;
    MGDP_HIP(hipStreamSynchronize(vi->stream));
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
        const size_t ev0 = vi->timed.tag.size();
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
        for (size_t i = ev0; i < vi->timed.tag.size(); ++i)  // sweeps past the stopping one no-op: not counted
            if (vi->timed.tag[i] > last) vi->timed.tag[i] = TimedPool::kUncounted;
        vi->k_done = last;
        vi->cur = last & 1;
        if (stop) break;
    }
    if (dv_out) *dv_out = dv;
    return 0;
}

// The sharded solve's all-reduce of one dV (mgdp_vi_solve_sharded).
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

// ---- what the protocol entry points share ----
// Before a solve's or an evaluation's first launch (mgdp_vi_reset, eval_begin; mgdp_vi_resume starts from it).
inline void protocol_state_reset(mgdp_vi *vi) {
    vi->fresh = 1;  // the next fused launch ignores kenv/dvenv and starts from V_0 = 0
    vi->cur = 0;
    vi->k_done = 0;
    vi->k_min = 0;
    vi->k_done_valid = false;
    vi->sweeps = 0;
    vi->converged = 0;
}
inline int not_evaluated(const mgdp_vi *vi) {
    MGDP_CHECK(!vi->evaluated, MGDP_E_INVALID, "the handle holds a policy evaluation: call mgdp_vi_reset first");
    return 0;
}
inline int device_protocol_supported(const mgdp_vi *vi) {
    MGDP_CHECK(vi->d.method == MGDP_METHOD_FUSED && !vi->plan.opts, MGDP_E_UNSUPPORTED,
               "the device protocol runs the fused method without horizon / lava options");
    return 0;
}

// The solve's closing steps, from the common sweep k with dV(k) = dv: the global rule (vi_rule.h; a
// finite horizon is exactly its H sweeps and runs none), finish, `converged` and the out-parameters.
// step(k + 1, &dv): every grid one sweep further.
template <typename Step>
int solve_close(mgdp_vi *vi, int32_t k, double dv, Step &&step, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    if (vi->d.horizon == 0)
        if (int rc = rule_sweeps(vi->d.tol, vi->d.max_sweeps, &k, &dv, step)) return rc;
    if (int rc = mgdp_vi_finish(vi, k)) return rc;
    vi->converged = rule_report(vi->d.horizon, vi->d.tol, k, dv, sweeps_out, dv_out, converged_out);
    return 0;
}
int solve_close(mgdp_vi *vi, int32_t k, double dv, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    return solve_close(vi, k, dv, [vi](int32_t, double *d) { return mgdp_vi_sweep(vi, d); }, sweeps_out, dv_out, converged_out);
}

// Resident server (lone grid or batch): a solve is a request word and a wait on host memory, so the
// steady state makes no HIP call at all (no device guard either); anything else -- a server
// that may be leaving, a finite horizon -- is left to the caller's general path (*served = false).
// (a batch whose learned dispatch order is due takes the general path: mgdp_vi_reset learns it)
int solve_served(mgdp_vi *vi, bool *served, int32_t *sweeps_out, double *dv_out, int32_t *converged_out) {
    *served = false;
    const bool learn_due = vi->d.B > 1 && !vi->order_valid && vi->kn.order_src == 2 && vi->solves_since_load > 0;
    if (!(vi->serving && served_eligible(vi) && vi->d.horizon == 0 && !learn_due)) return 0;
    const double idle_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - vi->serve_last).count();
    if (!(idle_us * 100.0 <= 0.5 * (double)vi->serve_idle_ticks)) return 0;
    *served = true;
    vi->cur = 0;
    vi->k_done = 0;
    vi->k_done_valid = false;
    post_request(vi);
    vi->fresh = 0;
    int32_t k = 0;
    if (int rc = reduce_env(vi, &k, nullptr)) return rc;
    vi->serve_last = std::chrono::steady_clock::now();
    double dv = vi->dv_red;
    // a batch is complete at K when every grid ended there or at an exact fixed point (mgdp_vi_run_to)
    const bool at_k = vi->d.B == 1 || vi->k_min == k || (vi->dv_red == 0.0 && vi->k_min > 0);
    if (vi->d.B > 1) ++vi->solves_since_load;
    if (at_k && (dv < vi->d.tol || k >= vi->d.max_sweeps)) {
        vi->k_done = k;
        vi->sweeps = k;
        vi->converged = rule_report(0, vi->d.tol, k, dv, sweeps_out, dv_out, converged_out);
        return 0;
    }
    // rounding broke the contraction: continue under the global rule on the general path
    if (int rc = mgdp_vi_run_to(vi, k, &dv)) return rc;
    return solve_close(vi, k, dv, sweeps_out, dv_out, converged_out);
}

}  // namespace
