// timed.h -- the pooled event pairs of timed launches, one implementation for both handles.
//
// Timed launches go through hipExtLaunchKernelGGL with a start/stop event pair, so the events carry
// the dispatch's own begin/end timestamps (what rocprofv3's kernel trace reports) rather than the
// times of separate marker packets.  Event pairs are pooled: no hipEventCreate once the pool is warm,
// and no runtime call at all with timing off.
#pragma once

#include <climits>
#include <utility>
#include <vector>

#include "common.h"

namespace mgdp {

struct TimedPair { hipEvent_t a = nullptr, b = nullptr; };

struct TimedPool {
    static constexpr int kUncounted = INT_MAX;  // a pending pair's tag set to this: collect() skips its time
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev, pool;  // pending pairs, free pairs
    std::vector<int> tag;                                     // the caller's tag of each pending pair
    double total_ms = 0.0;
    int64_t launches = 0;

    // The event pair of the next timed launch (null, null with timing off).
    int begin(int tag_, TimedPair *tp) {
        tp->a = tp->b = nullptr;
        if (!on) return 0;
        std::pair<hipEvent_t, hipEvent_t> e;
        if (!pool.empty()) {
            e = pool.back();
            pool.pop_back();
        } else {
            MGDP_HIP(hipEventCreate(&e.first));
            MGDP_HIP(hipEventCreate(&e.second));
        }
        ev.push_back(e);
        tag.push_back(tag_);
        tp->a = e.first;
        tp->b = e.second;
        return 0;
    }
    // Fold the completed pairs into total_ms / launches and hand them back to the pool (after a stream sync).
    int collect() {
        for (size_t i = 0; i < ev.size(); ++i) {
            if (tag[i] != kUncounted) {
                float ms = 0.f;
                MGDP_HIP(hipEventElapsedTime(&ms, ev[i].first, ev[i].second));
                total_ms += ms;
                launches += 1;
            }
            pool.push_back(ev[i]);
        }
        ev.clear();
        tag.clear();
        return 0;
    }
    // enable_timing: drop what was timed before this call (after a stream sync)
    int restart(bool on_) {
        if (int rc = collect()) return rc;
        on = on_;
        total_ms = 0.0;
        launches = 0;
        return 0;
    }
    // kernel_time (after a stream sync); each out-parameter may be null
    int read(double *ms_out, int64_t *launches_out) {
        if (int rc = collect()) return rc;
        if (ms_out) *ms_out = total_ms;
        if (launches_out) *launches_out = launches;
        return 0;
    }
    void destroy() {
        for (auto *v : {&ev, &pool}) {
            for (auto &p : *v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
            v->clear();
        }
        tag.clear();
    }
};

}  // namespace mgdp
