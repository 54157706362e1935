// envs_qlearn.h -- tabular Q-learning on resident envs; included into envs.hip
// inside namespace mgdp, after envs_rollout.h (the same translation unit as step_core).
//
//   envs_qlearn_kernel<MODEL, LDS, SLIP>  one lane per env, one wave per workgroup, as the rollout: every
//       env takes n_steps eps-greedy steps through step_core and updates its own fp64 table
//       Q[b][S][A] after each one; an episode that terminates or truncates restarts from the env's
//       record at call entry (the snapshot) inside the launch.  Nothing of the env is written back:
//       only Q, the explore streams, the slip streams (SLIP) and the outputs change.
//       LDS: the wave's planes are staged as in the rollout and the loop steps (and mutates) the LDS
//       copy; the plane in HBM is the snapshot, and a lane whose episode mutated its plane copies it
//       in again at the episode's end.  Otherwise the reader is the env's plane in HBM, which is never
//       written: XYD grids only (they never mutate); the host refuses DoorKey without LDS.
//   envs_q_greedy_kernel<A>  one thread per (b, s): the lowest-index argmax of Q[b][s][0..n_act) and,
//       optionally, that maximum.
//
// The explore stream of env b is a second set of section 17 records (SlipArgs' state / half part),
// seeded by envs_slip_seed_kernel.  Q rows are per-lane gathers in HBM / L2 (56 or 40 bytes a row): the
// greedy scan, the bootstrap scan and the update re-read memory every time, so the rule's order (the
// bootstrap is read before the update, the next step's scan after it) holds for s' == s as well.
#pragma once

struct QLearnArgs {
    double *Q;  // [B][S][A], A the model's lanes
    int S, n_steps, n_act, unit_goal, trace_len;
    double alpha, gamma, eps;
    int32_t *steps, *episodes, *wins;
    double *ret;
    int32_t *status;
    int32_t *tr_state;  // [trace_len][B] or null
    int8_t *tr_act;
};

// max over row[0..n_act) and its lowest index: scan from lane 0, replace on strict >.  All A entries
// of the row exist and are loaded (independent loads); those past n_act are not looked at.
template <int A>
__device__ __forceinline__ void q_row_max(const double *row, int n_act, double &best, int &arg) {
    best = row[0];
    arg = 0;
#pragma unroll
    for (int k = 1; k < A; ++k) {
        const double v = row[k];
        const bool up = k < n_act && v > best;
        best = up ? v : best;
        arg = up ? k : arg;
    }
}

// The rollout's staging pass (envs_rollout.h) a second time: the wave's planes are contiguous in HBM
// (n_env * HWp bytes from env e0) and go to LDS 16 bytes per lane and turn, at the odd-dword stride
// roll_stride; the model check's counts and the door index are gathered per env slot on the way.  The
// caller's __syncthreads() makes planes and counts visible.  envs_rollout_kernel keeps its inline form:
// calling this one there leaves every resource figure alone but reorders the four LDS instantiations'
// code, and two of their workloads then timed above the parent's spread (profiles/episode_sharing/).
struct PlaneScanShared {
    int bad[kRollWave], ndoor[kRollWave], door[kRollWave], doorcode[kRollWave], nkey[kRollWave], keyc[kRollWave];
    __device__ __forceinline__ PlaneScan of(int l) const {
        return PlaneScan{bad[l], ndoor[l], door[l], doorcode[l], nkey[l], keyc[l]};
    }
};

template <int MODEL>
__device__ __forceinline__ void stage_planes(PlaneScanShared &sh, unsigned char *smem, const uint8_t *CELL, int e0,
                                             int n_env, int HWp) {
    const int lane = threadIdx.x;
    const int stride = roll_stride(HWp);
    sh.bad[lane] = 0; sh.ndoor[lane] = 0; sh.door[lane] = 0; sh.doorcode[lane] = 0; sh.nkey[lane] = 0; sh.keyc[lane] = 0;
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(CELL + (long long)e0 * HWp);
    const int per = HWp >> 4;
    for (int i = lane; i < n_env * per; i += kRollWave) {
        const uint4 v = src[i];
        const int slot = i / per, off = (i - slot * per) << 4;
        uint32_t *dst = reinterpret_cast<uint32_t *>(smem + slot * stride + off);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        PlaneScan q{0, 0, 0, 0, 0, 0};
        scan_dword<MODEL>(v.x, off, q);
        scan_dword<MODEL>(v.y, off + 4, q);
        scan_dword<MODEL>(v.z, off + 8, q);
        scan_dword<MODEL>(v.w, off + 12, q);
        if (q.bad) atomicOr(&sh.bad[slot], 1);
        if (q.ndoor) { atomicAdd(&sh.ndoor[slot], q.ndoor); sh.door[slot] = q.door; sh.doorcode[slot] = q.doorcode; }
        if (q.nkey) { atomicAdd(&sh.nkey[slot], q.nkey); sh.keyc[slot] = q.keyc; }
    }
}

template <int MODEL, bool LDS, bool SLIP>
__global__ void __launch_bounds__(kRollWave)
envs_qlearn_kernel(EnvGeo g, const uint8_t *__restrict__ CELL, const int32_t *__restrict__ agent,
                   const int32_t *__restrict__ carry, const int32_t *__restrict__ max_steps, QLearnArgs q, SlipArgs ex,
                   SlipArgs sl) {
    static_assert(LDS || MODEL == kRollXYD, "the HBM reader has no copy to restore a mutated plane from");
    constexpr int A = MODEL == kRollXYD ? 7 : 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ PlaneScanShared sh;
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * kRollWave;
    const int e = e0 + lane;
    const int n_env = min(kRollWave, g.B - e0);
    const int stride = roll_stride(g.HWp);
    const bool mine = e < g.B;
    const uint8_t *snap = CELL + (long long)(mine ? e : e0) * g.HWp;  // this env's plane in HBM: the snapshot
    PlaneScan p{0, 0, 0, 0, 0, 0};
    uint8_t *lplane = nullptr;  // LDS: this env's live plane
    if (LDS) {
        stage_planes<MODEL>(sh, smem, CELL, e0, n_env, g.HWp);
        __syncthreads();
        p = sh.of(lane);
        lplane = smem + lane * stride;
    } else if (mine) {
        scan_plane_global<MODEL>(snap, g.HWp, p);
    }
    const uint8_t *plane = LDS ? lplane : snap;
    // the snapshot's registers: an episode starts here
    int x0 = 0, y0 = 0, d0 = 0, sc0 = 0, ct0 = 0, cc0 = 0, ms = 1;
    int status = MGDP_OK;
    if (mine) {
        const int4 ag = reinterpret_cast<const int4 *>(agent)[e];
        const int2 cr = reinterpret_cast<const int2 *>(carry)[e];
        x0 = ag.x; y0 = ag.y; d0 = ag.z; sc0 = ag.w; ct0 = cr.x; cc0 = cr.y;
        ms = max_steps[e];
        status = model_status<MODEL>(p, ct0, cc0);
    }
    const bool dopen0 = code_is_open_door(p.doorcode);
    int x = x0, y = y0, d = d0, sc = sc0, ct = ct0, cc = cc0;
    bool dopen = dopen0;
    int n = 0, episodes = 0, wins = 0, dirty = 0;
    double ret = 0.0;
    bool live = mine && status == MGDP_OK;
    // both streams stay in registers for the whole loop; an env outside the model draws nothing
    Pcg64 xr(U128{0, 0}, U128{0, 0}, false, 0u), sr(U128{0, 0}, U128{0, 0}, false, 0u);
    if (mine) xr = slip_load(ex, e);
    if (SLIP && mine) sr = slip_load(sl, e);
    double *Qb = q.Q + (long long)(mine ? e : e0) * q.S * A;
    const auto rd = [&](int cx, int cy, int &t, int &c, int &s) { cell_decode(plane[cy * g.W + cx], t, c, s); };
    // wave-uniform bound: the budget, or until no lane is live (a live lane's n equals it)
    for (int it = 0; it < q.n_steps && __ballot(live) != 0; ++it) {
        if (live) {
            const int s = state_of<MODEL>(g.W, x, y, d, ct, dopen);
            double *row = Qb + (long long)s * A;
            double best;
            int ln;
            q_row_max<A>(row, q.n_act, best, ln);
            const double u = xr.next_double();
            if (u < q.eps) ln = xr.integers(0, q.n_act);
            const int a = lane_action<MODEL>(ln);
            int ax = a;  // the learner updates the lane it chose, whatever the slip executes
            if (SLIP) ax = slip_decide(sr, sl.prob, sl.random_action, a);
            const StepOut o = step_core(g, rd, x, y, d, sc, ct, cc, ax, ms);
            if (o.stat != MGDP_OK) {  // the draws stay drawn, Q stays as it is
                status = o.stat;
                live = false;
            } else {
                if (it < q.trace_len) {
                    q.tr_state[(long long)it * g.B + e] = s;
                    q.tr_act[(long long)it * g.B + e] = (int8_t)ax;
                }
                if (LDS && o.mut) {  // the front cell as pickup / drop / toggle left it, in the LDS copy only
                    const int code = (int)cell_code(o.nt, o.nc, o.ns);
                    lplane[o.fi] = (uint8_t)code;
                    dirty = 1;
                    if (MODEL == kRollDoorKey && o.fi == p.door) dopen = code_is_open_door(code);
                }
                x = o.x; y = o.y; d = o.d; sc = o.sc; ct = o.ct; cc = o.cc;
                const int s2 = state_of<MODEL>(g.W, x, y, d, ct, dopen);
                double m;
                int lm;
                q_row_max<A>(Qb + (long long)s2 * A, q.n_act, m, lm);  // read before the update (s2 may be s)
                const double rl = (q.unit_goal && o.r > 0.0) ? 1.0 : o.r;
                double tgt = rl;
                if (!o.term) {  // a truncated step bootstraps
                    const double gm = q.gamma * m;
                    tgt = rl + gm;
                }
                const double qo = row[ln];
                const double df = tgt - qo;
                const double ad = q.alpha * df;
                row[ln] = qo + ad;
                n += 1;
                ret = ret + o.r;
                if (o.term | o.trunc) {  // back to the snapshot
                    episodes += 1;
                    wins += (o.term && o.r > 0.0) ? 1 : 0;
                    if (LDS && dirty) {
                        const uint4 *src = reinterpret_cast<const uint4 *>(snap);
                        for (int i = 0; i < (g.HWp >> 4); ++i) {
                            const uint4 v = src[i];
                            uint32_t *dst = reinterpret_cast<uint32_t *>(lplane + (i << 4));
                            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
                        }
                        dirty = 0;
                    }
                    x = x0; y = y0; d = d0; sc = sc0; ct = ct0; cc = cc0;
                    dopen = dopen0;
                }
            }
        }
    }
    if (mine) {
        q.steps[e] = n;
        q.episodes[e] = episodes;
        q.wins[e] = wins;
        q.ret[e] = ret;
        q.status[e] = status;
        slip_store(ex, e, xr);
        if (SLIP) slip_store(sl, e, sr);
    }
}

// pi[b][s] = the lowest-index argmax of Q[b][s][0..n_act), Vq[b][s] (or null) = that maximum; n = B * S rows.
template <int A>
__global__ void __launch_bounds__(256)
envs_q_greedy_kernel(long long n, const double *__restrict__ Q, int n_act, int8_t *__restrict__ pi,
                     double *__restrict__ Vq) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double best;
    int arg;
    q_row_max<A>(Q + i * A, n_act, best, arg);
    pi[i] = (int8_t)arg;
    if (Vq) Vq[i] = best;
}
