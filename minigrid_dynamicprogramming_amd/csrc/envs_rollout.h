// envs_rollout.h -- tabular policies executed on resident envs; included into
// envs.hip inside namespace mgdp, after step_core (the same translation unit, as vi_eval.h is for vi.hip).
//
//   envs_policy_actions_kernel<MODEL>   one lane per env: the state index of the live env in the order
//       of mgdp_vi_get_policy, the policy's lane there, the env action (-1: none) and a status.  No
//       stepping: its output is what mgdp_envs_step_device takes.
//   envs_rollout_kernel<MODEL, LDS, SLIP>  one lane per env, one wave per workgroup: every env is carried
//       through step_core until it terminates, truncates, fails or the budget ends -- no observation,
//       no launch per step, no host in the loop.  LDS: the wave's 64 cell planes are staged into LDS
//       with 16-byte loads (the model check and the DoorKey door index come out of the same pass), the
//       loop steps on LDS and the planes go back once at exit if any env mutated its grid.  Otherwise
//       the reader is the env's own plane in HBM (grids whose 64 planes do not fit a CU's LDS).
//       SLIP: every step's action first passes the env's own PCG64 stream -- kept
//       with probability prob, else random_action or integers(0, 6) -- held in registers for the whole
//       loop and written back at exit.
//   envs_slip_seed_kernel / envs_slip_actions_kernel  one lane per env: the stream of seed0 + b, and one
//       slip decision on a given action (for step_device loops that want observations).
//
// The LDS stride per env is HWp + 4 bytes: HWp is a multiple of 16, so the stride is an odd number of
// dwords and lane l's byte at the same cell offset falls into bank (l * odd + c) mod 32 -- distinct
// over each group of 32 lanes.  With the natural stride HWp (256 B for 16 x 16) every lane would hit
// one bank.
#pragma once

enum { kRollXYD = 0, kRollDoorKey = 1 };

struct RolloutArgs {
    const int8_t *pi;  // [T][B][S] action lanes
    int T, S, n_max, trace_len;
    int32_t *steps;
    double *ret;
    uint8_t *term, *trunc;
    int32_t *status;
    int32_t *tr_state;  // [trace_len][B] or null
    int8_t *tr_act;
};

// What the model check needs from one plane: a cell outside the model, the doors and the keys.
struct PlaneScan {
    int bad, ndoor, door, doorcode, nkey, keyc;
};

// Four cell codes (one dword, cells base .. base+3).  Plain cells are the XYD model's; the DoorKey
// model adds doors and keys, counted here and judged by model_status.
template <int MODEL>
__device__ __forceinline__ void scan_dword(uint32_t w, int base, PlaneScan &p) {
    constexpr uint32_t plain = (1u << T_EMPTY) | (1u << T_WALL) | (1u << T_FLOOR) | (1u << T_GOAL) | (1u << T_LAVA);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = (w >> (8 * k)) & 0xffu;
        const bool door = (c & 0x80u) != 0;
        const bool ok = !door && ((plain >> (c >> 3)) & 1u);
        if (MODEL == kRollXYD) {
            p.bad |= !ok;
        } else if (door) {
            p.ndoor += 1;
            p.door = base + k;
            p.doorcode = (int)c;
        } else if ((int)(c >> 3) == T_KEY) {
            p.nkey += 1;
            p.keyc = (int)(c & 7u);
        } else {
            p.bad |= !ok;
        }
    }
}

template <int MODEL>
__device__ __forceinline__ void scan_plane_global(const uint8_t *cell, int HWp, PlaneScan &p) {
    const uint4 *src = reinterpret_cast<const uint4 *>(cell);  // planes are 16-byte aligned (HWp % 16 == 0)
    for (int i = 0; i < (HWp >> 4); ++i) {
        const uint4 v = src[i];
        scan_dword<MODEL>(v.x, 16 * i, p);
        scan_dword<MODEL>(v.y, 16 * i + 4, p);
        scan_dword<MODEL>(v.z, 16 * i + 8, p);
        scan_dword<MODEL>(v.w, 16 * i + 12, p);
    }
}

// XYD: plain cells, nothing carried.  DoorKey: plain cells plus exactly one door and its key, the key
// on the grid or in the agent's hands, and nothing else carried.
template <int MODEL>
__device__ __forceinline__ int model_status(const PlaneScan &p, int ct, int cc) {
    if (MODEL == kRollXYD) return (p.bad || ct != 0) ? MGDP_E_UNSUPPORTED : MGDP_OK;
    const int doorc = p.doorcode & 7;
    const bool key_ok = (ct == 0 && p.nkey == 1 && p.keyc == doorc) || (ct == T_KEY && p.nkey == 0 && cc == doorc);
    return (p.bad || p.ndoor != 1 || !key_ok) ? MGDP_E_UNSUPPORTED : MGDP_OK;
}

__device__ __forceinline__ bool code_is_open_door(int code) { return (code & 0x80) && ((code >> 3) & 3) == D_OPEN; }

template <int MODEL>
__device__ __forceinline__ int state_of(int W, int x, int y, int d, int ct, bool dopen) {
    const int s = (y * W + x) * 4 + d;
    return MODEL == kRollXYD ? s : (s * 2 + (ct == T_KEY ? 1 : 0)) * 2 + (dopen ? 1 : 0);
}

// Lane -> env action: XYD lanes are the actions; DoorKey lanes 0..4 = (left, right, forward, pickup, toggle).
template <int MODEL>
__device__ __forceinline__ int lane_action(int lane) {
    return MODEL == kRollXYD ? lane : lane + (lane == 4 ? 1 : 0);
}
template <int MODEL>
__device__ __forceinline__ bool lane_ok(int lane) {
    return (unsigned)lane < (MODEL == kRollXYD ? 7u : 5u);
}

template <int MODEL>
__global__ void __launch_bounds__(256)
envs_policy_actions_kernel(EnvGeo g, const uint8_t *__restrict__ CELL, const int32_t *__restrict__ agent,
                           const int32_t *__restrict__ carry, const int8_t *__restrict__ pi, int T, int S,
                           int32_t *__restrict__ actions, int32_t *__restrict__ status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.B) return;
    const int4 ag = reinterpret_cast<const int4 *>(agent)[e];
    const int2 cr = reinterpret_cast<const int2 *>(carry)[e];
    PlaneScan p{0, 0, 0, 0, 0, 0};
    scan_plane_global<MODEL>(CELL + (long long)e * g.HWp, g.HWp, p);
    int st = model_status<MODEL>(p, cr.x, cr.y);
    int a = -1;
    if (st == MGDP_OK) {
        if (T > 1 && (unsigned)ag.w >= (unsigned)T) {
            st = MGDP_E_INVALID;
        } else {
            const int s = state_of<MODEL>(g.W, ag.x, ag.y, ag.z, cr.x, code_is_open_door(p.doorcode));
            const int lane = pi[((long long)(T > 1 ? ag.w : 0) * g.B + e) * S + s];
            if (lane_ok<MODEL>(lane)) a = lane_action<MODEL>(lane);
            else st = MGDP_E_ACTION;
        }
    }
    actions[e] = a;
    status[e] = st;
}

constexpr int kRollWave = 64;  // envs per workgroup: one wave
__host__ __device__ inline int roll_stride(int HWp) { return HWp + 4; }

// ---- slip streams -----------------------------------------------------------
// Env b's record: state[4 b ..] = (state hi, state lo, inc hi, inc lo), half[2 b ..] = (has_uint32, uinteger).
struct SlipArgs {
    double prob;
    int random_action;  // -1: integers(0, 6)
    uint64_t *state;
    uint32_t *half;
};

__device__ __forceinline__ Pcg64 slip_load(const SlipArgs &sl, int e) {
    const ulonglong2 st = reinterpret_cast<const ulonglong2 *>(sl.state)[2 * (long long)e];
    const ulonglong2 in = reinterpret_cast<const ulonglong2 *>(sl.state)[2 * (long long)e + 1];
    const uint2 h = reinterpret_cast<const uint2 *>(sl.half)[e];
    return Pcg64(U128{st.x, st.y}, U128{in.x, in.y}, h.x != 0, h.y);
}
// The increment never changes: the state and the half-word go back.  numpy keeps the last buffered
// half in uinteger after it is consumed, and so does buf.
__device__ __forceinline__ void slip_store(const SlipArgs &sl, int e, const Pcg64 &r) {
    reinterpret_cast<ulonglong2 *>(sl.state)[2 * (long long)e] = make_ulonglong2(r.state.hi, r.state.lo);
    reinterpret_cast<uint2 *>(sl.half)[e] = make_uint2(r.has32 ? 1u : 0u, r.buf);
}
// One slip decision: u = random(); u < prob keeps the action, else random_action or integers(0, 6).
__device__ __forceinline__ int slip_decide(Pcg64 &r, double prob, int random_action, int a) {
    const double u = r.next_double();
    if (u < prob) return a;
    return random_action >= 0 ? random_action : r.integers(0, 6);
}

__global__ void __launch_bounds__(256)
envs_slip_seed_kernel(int B, uint64_t seed0, const uint8_t *__restrict__ mask, SlipArgs sl) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B || (mask && !mask[e])) return;
    const Pcg64 r(seed0 + (uint64_t)e);
    reinterpret_cast<ulonglong2 *>(sl.state)[2 * (long long)e + 1] = make_ulonglong2(r.inc.hi, r.inc.lo);
    slip_store(sl, e, r);
}

// in == out is allowed (each lane reads its entry before it writes it).  A negative action is
// policy_actions' "none": it passes through and draws nothing, as a failed lookup does in the rollout.
__global__ void __launch_bounds__(256)
envs_slip_actions_kernel(int B, SlipArgs sl, const int32_t *in, int32_t *out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    int a = in[e];
    if (a >= 0) {
        Pcg64 r = slip_load(sl, e);
        a = slip_decide(r, sl.prob, sl.random_action, a);
        slip_store(sl, e, r);
    }
    out[e] = a;
}

template <int MODEL, bool LDS, bool SLIP>
__global__ void __launch_bounds__(kRollWave)
envs_rollout_kernel(EnvGeo g, uint8_t *__restrict__ CELL, int32_t *__restrict__ agent, int32_t *__restrict__ carry,
                    const int32_t *__restrict__ max_steps, RolloutArgs r, SlipArgs sl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_bad[kRollWave], s_ndoor[kRollWave], s_door[kRollWave], s_doorcode[kRollWave], s_nkey[kRollWave],
        s_keyc[kRollWave];
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * kRollWave;
    const int e = e0 + lane;
    const int n_env = min(kRollWave, g.B - e0);
    const int stride = roll_stride(g.HWp);
    const bool mine = e < g.B;
    PlaneScan p{0, 0, 0, 0, 0, 0};
    uint8_t *plane;  // this env's cells: LDS or HBM
    if (LDS) {
        s_bad[lane] = 0; s_ndoor[lane] = 0; s_door[lane] = 0; s_doorcode[lane] = 0; s_nkey[lane] = 0; s_keyc[lane] = 0;
        __syncthreads();
        // the wave's planes are contiguous in HBM: n_env * HWp bytes from env e0, 16 bytes per lane and turn
        const uint4 *src = reinterpret_cast<const uint4 *>(CELL + (long long)e0 * g.HWp);
        const int per = g.HWp >> 4;
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
            if (q.bad) atomicOr(&s_bad[slot], 1);
            if (q.ndoor) { atomicAdd(&s_ndoor[slot], q.ndoor); s_door[slot] = q.door; s_doorcode[slot] = q.doorcode; }
            if (q.nkey) { atomicAdd(&s_nkey[slot], q.nkey); s_keyc[slot] = q.keyc; }
        }
        __syncthreads();
        p = PlaneScan{s_bad[lane], s_ndoor[lane], s_door[lane], s_doorcode[lane], s_nkey[lane], s_keyc[lane]};
        plane = smem + lane * stride;
    } else {
        plane = CELL + (long long)(mine ? e : e0) * g.HWp;
        if (mine) scan_plane_global<MODEL>(plane, g.HWp, p);
    }
    int x = 0, y = 0, d = 0, sc = 0, ct = 0, cc = 0, ms = 1;
    int status = MGDP_OK;
    if (mine) {
        const int4 ag = reinterpret_cast<const int4 *>(agent)[e];
        const int2 cr = reinterpret_cast<const int2 *>(carry)[e];
        x = ag.x; y = ag.y; d = ag.z; sc = ag.w; ct = cr.x; cc = cr.y;
        ms = max_steps[e];
        status = model_status<MODEL>(p, ct, cc);
    }
    bool dopen = code_is_open_door(p.doorcode);
    int n = 0, term = 0, trunc = 0, dirty = 0;
    double ret = 0.0;
    bool live = mine && status == MGDP_OK;
    Pcg64 rng(U128{0, 0}, U128{0, 0}, false, 0u);  // SLIP: the env's stream, in registers for the whole loop
    if (SLIP && mine) rng = slip_load(sl, e);
    const auto rd = [&](int cx, int cy, int &t, int &c, int &s) { cell_decode(plane[cy * g.W + cx], t, c, s); };
    // wave-uniform bound: until no lane is live or the budget is reached (a live lane's n equals it)
    for (int it = 0; (r.n_max <= 0 || it < r.n_max) && __ballot(live) != 0; ++it) {
        if (live) {
            const int s = state_of<MODEL>(g.W, x, y, d, ct, dopen);
            const bool t_ok = r.T == 1 || (unsigned)sc < (unsigned)r.T;
            const int ln = t_ok ? r.pi[((long long)(r.T > 1 ? sc : 0) * g.B + e) * r.S + s] : -1;
            int a = lane_action<MODEL>(ln);
            StepOut o{};
            if (!t_ok) o.stat = MGDP_E_INVALID;
            else if (!lane_ok<MODEL>(ln)) o.stat = MGDP_E_ACTION;
            else {  // a failed lookup draws nothing; a draw is never rolled back
                if (SLIP) a = slip_decide(rng, sl.prob, sl.random_action, a);
                o = step_core(g, rd, x, y, d, sc, ct, cc, a, ms);
            }
            if (o.stat != MGDP_OK) {  // the env is left as it was
                status = o.stat;
                live = false;
            } else {
                if (it < r.trace_len) {
                    r.tr_state[(long long)it * g.B + e] = s;
                    r.tr_act[(long long)it * g.B + e] = (int8_t)a;
                }
                if (o.mut) {  // the front cell as pickup / drop / toggle left it
                    const int code = (int)cell_code(o.nt, o.nc, o.ns);
                    plane[o.fi] = (uint8_t)code;
                    dirty = 1;
                    if (MODEL == kRollDoorKey && o.fi == p.door) dopen = code_is_open_door(code);
                }
                x = o.x; y = o.y; d = o.d; sc = o.sc; ct = o.ct; cc = o.cc;
                n += 1;
                ret = ret + o.r;
                term = o.term; trunc = o.trunc;
                if (term | trunc) live = false;
            }
        }
    }
    if (mine) {
        reinterpret_cast<int4 *>(agent)[e] = make_int4(x, y, d, sc);
        reinterpret_cast<int2 *>(carry)[e] = make_int2(ct, cc);
        r.steps[e] = n;
        r.ret[e] = ret;
        r.term[e] = (uint8_t)term;
        r.trunc[e] = (uint8_t)trunc;
        r.status[e] = status;
        if (SLIP) slip_store(sl, e, rng);
    }
    if (LDS && __ballot(dirty) != 0) {  // some env of the wave changed its grid: the planes go back once
        __syncthreads();
        uint4 *dstg = reinterpret_cast<uint4 *>(CELL + (long long)e0 * g.HWp);
        const int per = g.HWp >> 4;
        for (int i = lane; i < n_env * per; i += kRollWave) {
            const int slot = i / per, off = (i - slot * per) << 4;
            const uint32_t *sp = reinterpret_cast<const uint32_t *>(smem + slot * stride + off);
            dstg[i] = make_uint4(sp[0], sp[1], sp[2], sp[3]);
        }
    }
}
