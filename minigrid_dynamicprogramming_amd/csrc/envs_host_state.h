// envs_host_state.h -- what a handle holds, in and out: load (whole or masked), get / set state and the
// Box contents planes.  Every conversion between Grid.encode() layout and a plane is envs_codec.h's;
// here are the checks' wording, the copies and the masked load's launch.  Part of envs.hip (see envs_host.h).
#pragma once

namespace {

// A refused conversion in the entry points' words.
int codec_fail(const CodecError &e) {
    switch (e.kind) {
    case CodecError::not_a_cell:
        set_error("env %d cell (%d,%d): encoding (%d,%d,%d) is not a Grid.encode() cell", e.b, e.x, e.y, e.t, e.c, e.s);
        break;
    case CodecError::not_an_object:
        if (e.carried) set_error("env %d: carried contents (%d,%d,%d) is not an object encoding", e.b, e.t, e.c, e.s);
        else set_error("env %d cell (%d,%d): contents (%d,%d,%d) is not an object encoding", e.b, e.x, e.y, e.t, e.c, e.s);
        break;
    case CodecError::not_on_a_box:
        if (e.carried) set_error("env %d: contents for a carried non-box", e.b);
        else set_error("env %d cell (%d,%d): contents on a non-box cell", e.b, e.x, e.y);
        break;
    case CodecError::ok: return 0;
    }
    return MGDP_E_INVALID;
}

// The host packs every env's prepared record into one buffer in the staging layout (envs_codec.h).  A
// whole load copies its sections to the handle's buffers.  A masked reset (auto-reset of some envs)
// takes the buffer to the device in one copy and envs_masked_load_kernel writes the masked envs from it
// -- O(1) runtime calls for any number of envs (a per-env copy / memset loop made a 65536-env auto-reset
// ~300k API calls).  New grids hold no Box contents until mgdp_envs_set_contents says so.
int state_load(mgdp_envs *E, const uint8_t *enc, const int32_t *agent, const int32_t *max_steps, const uint8_t *see_through,
               const uint8_t *mask) {
    const int B = E->B, HWp = E->HWp;
    for (int b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        MGDP_CHECK(max_steps[b] > 0, MGDP_E_INVALID, "env %d: max_steps must be > 0", b);
        const int x = agent[3 * b], y = agent[3 * b + 1], d = agent[3 * b + 2];
        MGDP_CHECK(agent_in_grid(x, y, d, E->W, E->H), MGDP_E_BOUNDS, "env %d: agent (%d,%d,%d) outside the grid", b, x, y, d);
    }
    const StageLayout L{B, HWp};
    std::vector<uint8_t> stage(L.total(), 0);  // carry: nothing
    uint8_t *st = stage.data();
    int32_t *ag = L.agent(st);
    for (int b = 0; b < B; ++b) {
        st[L.mask(b)] = !mask || mask[b];
        st[L.see(b)] = see_through[b];
        if (!mask || mask[b]) { ag[4 * b] = agent[3 * b]; ag[4 * b + 1] = agent[3 * b + 1]; ag[4 * b + 2] = agent[3 * b + 2]; }
    }
    if (CodecError err = encode_cells(env_shape(E), enc, mask, L.cells(st))) return codec_fail(err);
    std::memcpy(L.max(st), max_steps, sizeof(int32_t) * B);
    if (!mask) {
        if (E->d_cont) {
            MGDP_HIP(hipMemsetAsync(E->d_cont, 0, (size_t)B * HWp, E->stream));
            MGDP_HIP(hipMemsetAsync(E->d_ccont, 0, (size_t)B, E->stream));
        }
        MGDP_HIP(hipMemcpyAsync(E->d_cell, L.cells(st), (size_t)B * HWp, hipMemcpyHostToDevice, E->stream));
        MGDP_HIP(hipMemcpyAsync(E->d_agent, ag, sizeof(int32_t) * 4 * B, hipMemcpyHostToDevice, E->stream));
        MGDP_HIP(hipMemcpyAsync(E->d_carry, L.carry(st), sizeof(int32_t) * 2 * B, hipMemcpyHostToDevice, E->stream));
        MGDP_HIP(hipMemcpyAsync(E->d_max, L.max(st), sizeof(int32_t) * B, hipMemcpyHostToDevice, E->stream));
        MGDP_HIP(hipMemcpyAsync(E->d_see, &st[L.see(0)], B, hipMemcpyHostToDevice, E->stream));
    } else {
        if (int rc = grow(E, E->stage, L.total())) return rc;
        MGDP_HIP(hipMemcpyAsync(E->stage.p, st, L.total(), hipMemcpyHostToDevice, E->stream));
        hipLaunchKernelGGL(envs_masked_load_kernel, dim3(B), dim3(64), 0, E->stream, B, HWp, E->stage.p, E->d_cell,
                           E->d_agent, E->d_carry, E->d_max, E->d_see, E->d_cont, E->d_ccont);
        MGDP_HIP(hipGetLastError());
    }
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

int state_get(mgdp_envs *E, uint8_t *enc, int32_t *agent, int32_t *carry, int32_t *step_count) {
    const int B = E->B;
    std::vector<int32_t> ag((size_t)B * 4);
    std::vector<uint8_t> cl(enc ? (size_t)B * E->HWp : 0);
    MGDP_HIP(hipMemcpyAsync(ag.data(), E->d_agent, ag.size() * 4, hipMemcpyDeviceToHost, E->stream));
    if (download(E, carry, E->d_carry, 8 * (size_t)B) || download(E, enc ? cl.data() : nullptr, E->d_cell, cl.size()))
        return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    for (int b = 0; b < B; ++b) {
        if (agent) { agent[3 * b] = ag[4 * b]; agent[3 * b + 1] = ag[4 * b + 1]; agent[3 * b + 2] = ag[4 * b + 2]; }
        if (step_count) step_count[b] = ag[4 * b + 3];
    }
    if (enc) decode_cells(env_shape(E), cl.data(), enc);
    return 0;
}

int state_set(mgdp_envs *E, const int32_t *agent, const int32_t *carry, const int32_t *step_count, const uint8_t *mask) {
    const int B = E->B;
    std::vector<int32_t> ag((size_t)B * 4), cr((size_t)B * 2);
    std::vector<uint8_t> cc((carry && E->d_ccont) ? (size_t)B : 0);  // carried Box contents
    MGDP_HIP(hipMemcpyAsync(ag.data(), E->d_agent, ag.size() * 4, hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipMemcpyAsync(cr.data(), E->d_carry, cr.size() * 4, hipMemcpyDeviceToHost, E->stream));
    if (!cc.empty()) MGDP_HIP(hipMemcpyAsync(cc.data(), E->d_ccont, cc.size(), hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    for (int b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        if (agent) {
            MGDP_CHECK(agent_in_grid(agent[3 * b], agent[3 * b + 1], agent[3 * b + 2], E->W, E->H), MGDP_E_BOUNDS,
                       "env %d: agent outside the grid", b);
            ag[4 * b] = agent[3 * b]; ag[4 * b + 1] = agent[3 * b + 1]; ag[4 * b + 2] = agent[3 * b + 2];
        }
        if (step_count) ag[4 * b + 3] = step_count[b];
        if (carry) {
            cr[2 * b] = carry[2 * b]; cr[2 * b + 1] = carry[2 * b + 1];
            if (!cc.empty()) cc[b] = 0;  // a new carry holds nothing (see contents_set)
        }
    }
    MGDP_HIP(hipMemcpyAsync(E->d_agent, ag.data(), ag.size() * 4, hipMemcpyHostToDevice, E->stream));
    MGDP_HIP(hipMemcpyAsync(E->d_carry, cr.data(), cr.size() * 4, hipMemcpyHostToDevice, E->stream));
    if (!cc.empty()) MGDP_HIP(hipMemcpyAsync(E->d_ccont, cc.data(), cc.size(), hipMemcpyHostToDevice, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

// Box(contains=...) (world_object.py:272-294): toggle puts the held object in the box's cell,
// pickup carries the box with it, drop puts it back.  Contents are (type, colour, state) triples in
// Grid.encode() layout, type <= 1 (unseen / empty) = nothing held; each must be a cell code (see
// cell_code) and sit on a Box cell of the current grid; a carried one needs a carried Box.
int contents_set(mgdp_envs *E, const uint8_t *contents, const int32_t *carry_contents) {
    const int B = E->B, HWp = E->HWp;
    std::vector<uint8_t> cl((size_t)B * HWp);
    std::vector<int32_t> cr((size_t)B * 2);
    MGDP_HIP(hipMemcpyAsync(cl.data(), E->d_cell, cl.size(), hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipMemcpyAsync(cr.data(), E->d_carry, cr.size() * 4, hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    std::vector<uint8_t> co(contents ? (size_t)B * HWp : 0), cc(carry_contents ? (size_t)B : 0);
    if (contents)
        if (CodecError err = encode_contents(env_shape(E), contents, cl.data(), co.data())) return codec_fail(err);
    if (carry_contents)
        if (CodecError err = encode_carried(B, carry_contents, cr.data(), cc.data())) return codec_fail(err);
    if (!E->d_cont) {
        hipError_t e = hipMalloc((void **)&E->d_cont, (size_t)B * HWp);
        if (e == hipSuccess) e = hipMalloc((void **)&E->d_ccont, (size_t)B);
        if (e == hipSuccess) e = hipMemsetAsync(E->d_cont, 0, (size_t)B * HWp, E->stream);
        if (e == hipSuccess) e = hipMemsetAsync(E->d_ccont, 0, (size_t)B, E->stream);
        if (e != hipSuccess) {
            (void)hipFree(E->d_cont);
            (void)hipFree(E->d_ccont);
            E->d_cont = E->d_ccont = nullptr;
            return hip_fail(e, "mgdp_envs_set_contents allocation", __FILE__, __LINE__);
        }
    }
    if (contents) MGDP_HIP(hipMemcpyAsync(E->d_cont, co.data(), co.size(), hipMemcpyHostToDevice, E->stream));
    if (carry_contents) MGDP_HIP(hipMemcpyAsync(E->d_ccont, cc.data(), cc.size(), hipMemcpyHostToDevice, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

int contents_get(mgdp_envs *E, uint8_t *contents, int32_t *carry_contents) {
    const int B = E->B;
    std::vector<uint8_t> co((size_t)B * E->HWp, 0), cc((size_t)B, 0);
    if (E->d_cont) {
        MGDP_HIP(hipMemcpyAsync(co.data(), E->d_cont, co.size(), hipMemcpyDeviceToHost, E->stream));
        MGDP_HIP(hipMemcpyAsync(cc.data(), E->d_ccont, cc.size(), hipMemcpyDeviceToHost, E->stream));
        MGDP_HIP(hipStreamSynchronize(E->stream));
    }
    if (contents) decode_contents(env_shape(E), co.data(), contents);
    if (carry_contents) decode_carried(B, cc.data(), carry_contents);
    return 0;
}

}  // namespace
