// envs_host.h -- the env handle: struct mgdp_envs (the ABI's opaque handle), the kernel arguments made of
// it (env_geo, env_shape), launch_timed (every timed launch of the env half), the step launch, the
// device-to-host copy of an optional output, and the device buffers grown on demand (grow, RollCursor).
// Part of the single translation unit envs.hip: included after the device code, first of the host
// pieces (envs_host.h, envs_host_state.h, envs_host_episode.h, in this order).
#pragma once

// One set of per-env PCG64 records, allocated by its first seeding.
struct StreamTable {
    uint64_t *state = nullptr;  // [B][4] state hi, lo, inc hi, lo
    uint32_t *half = nullptr;   // [B][2] has_uint32, uinteger
    bool on = false;            // seeded: until then a seeding takes no mask
};

// A device buffer grown on demand (grow), never shrunk.
struct Scratch {
    uint8_t *p = nullptr;
    size_t bytes = 0;
};

struct mgdp_envs {
    int device = 0, B = 0, W = 0, H = 0, HW = 0, HWp = 0, vs = 7;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint8_t *d_cell = nullptr, *d_see = nullptr;  // d_cell: one-byte cell codes [B][HWp]
    uint8_t *d_cont = nullptr, *d_ccont = nullptr;  // Box contents planes (mgdp_envs_set_contents), else null
    int32_t *d_agent = nullptr, *d_carry = nullptr, *d_max = nullptr, *d_act = nullptr, *d_dir = nullptr,
            *d_status = nullptr;
    uint8_t *d_obs = nullptr, *d_term = nullptr, *d_trunc = nullptr;
    double *d_rew = nullptr;
    uint32_t nd_mask = 0;
    double death_cost = -1.0;
    int group = 2;  // lanes per env in envs_step_kernel (MGDP_STEP_GROUP = 1, 2, 4 or 8; 2 measured fastest)
    // stage: masked loads (auto-reset of some envs), one staging copy + envs_masked_load_kernel;
    // roll: the episode entry points' host-call scratch (the policy, Q, the trace; RollCursor)
    Scratch stage, roll;
    int roll_reader = -1;  // -1 = LDS planes whenever 64 of them fit, 0 / 1 = MGDP_ROLLOUT_READER=hbm / lds
    // the slip streams and Q-learning's explore streams (section 18)
    StreamTable slip, explore;
    double slip_p = 1.0;
    int slip_ra = -1;
    uint8_t *d_stream_mask = nullptr;  // [B] a masked reseed's mask (either table)
    TimedPool timed;  // kernel timing (mgdp_envs_enable_timing; timed.h)
};

namespace {

EnvGeo env_geo(const mgdp_envs *E) { return EnvGeo{E->B, E->W, E->H, E->HWp, E->vs, E->nd_mask, E->death_cost}; }
BatchShape env_shape(const mgdp_envs *E) { return BatchShape{E->B, E->W, E->H, E->HWp}; }

// Every launch the handle times: with timing on it carries a pooled event pair, at most 4096 of them
// pending (then the stream is drained and they are collected); with timing off it is the launch alone.
template <typename K, typename... Args>
int launch_timed(mgdp_envs *E, K k, dim3 grid, dim3 block, int smem, const Args &...args) {
    if (E->timed.ev.size() >= 4096) {
        MGDP_HIP(hipStreamSynchronize(E->stream));
        if (int rc = E->timed.collect()) return rc;
    }
    TimedPair tp;
    if (int rc = E->timed.begin(0, &tp)) return rc;
    hipExtLaunchKernelGGL(k, grid, block, smem, E->stream, tp.a, tp.b, 0, args...);
    MGDP_HIP(hipGetLastError());
    return 0;
}

int launch_step(mgdp_envs *E, const int32_t *d_act, uint8_t *d_obs, int32_t *d_dir, double *d_rew,
                uint8_t *d_term, uint8_t *d_trunc, int32_t *d_status, int observe_only) {
    const int ne = kGroupBlock / E->group;
    const int grid = (E->B + ne - 1) / ne;
    const int smem = (int)round_up(ne * E->vs * E->vs * 3, 16) + ne * ((E->vs + 1) * kWinRow + 4);
    auto pick = [&](auto k7, auto k5, auto k3) { return E->vs == 7 ? k7 : E->vs == 5 ? k5 : k3; };
    auto k = E->group == 8   ? pick(envs_step_kernel<7, 8>, envs_step_kernel<5, 8>, envs_step_kernel<3, 8>)
             : E->group == 4 ? pick(envs_step_kernel<7, 4>, envs_step_kernel<5, 4>, envs_step_kernel<3, 4>)
             : E->group == 1 ? pick(envs_step_kernel<7, 1>, envs_step_kernel<5, 1>, envs_step_kernel<3, 1>)
                             : pick(envs_step_kernel<7, 2>, envs_step_kernel<5, 2>, envs_step_kernel<3, 2>);
    return launch_timed(E, k, dim3(grid), dim3(kGroupBlock), smem, env_geo(E), E->d_cell, E->d_agent, E->d_carry, E->d_cont,
                        E->d_ccont, E->d_max, E->d_see, d_act, d_obs, d_dir, d_rew, d_term, d_trunc, d_status, observe_only);
}

// One device-to-host copy on the handle's stream; a null dst is an output the caller did not ask for.
int download(mgdp_envs *E, void *dst, const void *src, size_t bytes) {
    if (dst) MGDP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, E->stream));
    return 0;
}

// s holds at least `need` bytes; a buffer that may be in use leaves only once the stream is drained.
int grow(mgdp_envs *E, Scratch &s, size_t need) {
    if (s.bytes >= need) return 0;
    if (s.p) {
        MGDP_HIP(hipStreamSynchronize(E->stream));
        MGDP_HIP(hipFree(s.p));
    }
    s.p = nullptr;
    s.bytes = 0;
    MGDP_HIP(hipMalloc((void **)&s.p, need));
    s.bytes = need;
    return 0;
}

// A bump allocator over the roll scratch: take() lays the pieces of a host call out, each from a
// 16-byte boundary; grow(E, E->roll, end) then makes it hold them all, and roll_at<T>() is a piece's address.
struct RollCursor {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t off = end;
        end += round_up(bytes, 16);
        return off;
    }
};
template <typename T>
T *roll_at(const mgdp_envs *E, size_t off) { return reinterpret_cast<T *>(E->roll.p + off); }

}  // namespace
