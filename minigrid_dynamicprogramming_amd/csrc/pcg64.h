// pcg64.h -- numpy's Generator(PCG64(SeedSequence(seed))) restated for the device; shared by gen.hip
// (reset(seed) grid generation) and envs.hip (the slip streams of DESIGN.md section 17).
//   SeedSequence(entropy).generate_state(4, uint64)  -- numpy/random/bit_generator.pyx
//   PCG64 (XSL-RR 128/64, set_seed = srandom_r(state=w0:w1, seq=w2:w3)), next_uint32 hands out the
//     low then the high half of one 64-bit output (numpy/random/src/pcg64)
//   Generator.random() = (next_uint64 >> 11) * 2^-53; it never touches the buffered half-word
//   Generator.integers(lo, hi) for int64: range r = hi-lo-1; r == 0 -> lo without a draw; else
//     Lemire's bounded method on next_uint32 with the (2^32 - 1 - r) % (r + 1) rejection threshold
//   Generator.shuffle(list): for i = n-1..1: swap(i, random_interval(i)), random_interval = masked
//     next_uint32 rejection
// Pinned against numpy itself by tests/test_rng_restatement.py and tests/test_gpu_gen.py.
#pragma once

#include "common.h"

namespace mgdp {

struct U128 {
    uint64_t hi, lo;
};

__device__ __forceinline__ U128 mul128(U128 a, U128 b) {  // mod 2^128
    U128 r;
    r.lo = a.lo * b.lo;
    r.hi = __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
    return r;
}
__device__ __forceinline__ U128 add128(U128 a, U128 b) {
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
    return r;
}

// SeedSequence(seed).generate_state(4, np.uint64), pool size 4, no spawn key.
__device__ inline void seedseq_state(uint64_t seed, uint64_t (&out)[4]) {
    constexpr uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
    constexpr uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    uint32_t ent[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int nent = (seed >> 32) ? 2 : 1;  // _int_to_uint32_array: little-endian words, 0 -> [0]
    uint32_t hc = INIT_A;
    auto hashmix = [&](uint32_t v) {
        v ^= hc;
        hc *= MULT_A;
        v *= hc;
        v ^= v >> 16;
        return v;
    };
    auto mix = [](uint32_t x, uint32_t y) {
        uint32_t r = MIX_L * x - MIX_R * y;
        r ^= r >> 16;
        return r;
    };
    uint32_t pool[4];
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < nent ? ent[i] : 0u);
    for (int s = 0; s < 4; ++s)
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    uint32_t h = INIT_B;
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3];
        v ^= h;
        h *= MULT_B;
        v *= h;
        v ^= v >> 16;
        w[i] = v;
    }
    for (int i = 0; i < 4; ++i) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

struct Pcg64 {
    U128 state, inc;
    uint32_t buf;
    bool has32;

    __device__ void step() {
        const U128 mult{0x2360ED051FC65DA4ull, 0x4385DF649FCCF645ull};
        state = add128(mul128(state, mult), inc);
    }
    // a stream continued from its record (state, increment, buffered half-word)
    __device__ Pcg64(U128 st, U128 in, bool has, uint32_t half) : state(st), inc(in), buf(half), has32(has) {}
    __device__ explicit Pcg64(uint64_t seed) {
        uint64_t v[4];
        seedseq_state(seed, v);
        const U128 initstate{v[0], v[1]}, initseq{v[2], v[3]};
        inc = U128{(initseq.hi << 1) | (initseq.lo >> 63), (initseq.lo << 1) | 1u};
        state = U128{0, 0};
        step();
        state = add128(state, initstate);
        step();
        has32 = false;
        buf = 0;
    }
    __device__ uint64_t next64() {
        step();
        const uint64_t x = state.hi ^ state.lo;
        const unsigned rot = (unsigned)(state.hi >> 58);
        return (x >> rot) | (x << ((64u - rot) & 63u));
    }
    __device__ uint32_t next32() {
        if (has32) {
            has32 = false;
            return buf;
        }
        const uint64_t n = next64();
        has32 = true;
        buf = (uint32_t)(n >> 32);
        return (uint32_t)n;
    }
    // Generator.random(): 53 bits of one 64-bit draw; the product is exact
    __device__ double next_double() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
    // Generator.integers(lo, hi) (int64, hi exclusive, hi - lo <= 2^32)
    __device__ int integers(int lo, int hi) {
        const uint32_t rng = (uint32_t)(hi - lo - 1);
        if (rng == 0) return lo;
        const uint32_t excl = rng + 1u;
        uint64_t m = (uint64_t)next32() * excl;
        uint32_t left = (uint32_t)m;
        if (left < excl) {
            const uint32_t thr = (0xFFFFFFFFu - rng) % excl;
            while (left < thr) {
                m = (uint64_t)next32() * excl;
                left = (uint32_t)m;
            }
        }
        return lo + (int)(m >> 32);
    }
    // random_interval(max), the draw of Generator.shuffle on lists
    __device__ int interval(int mx) {
        if (mx == 0) return 0;
        uint32_t mask = (uint32_t)mx;
        mask |= mask >> 1;
        mask |= mask >> 2;
        mask |= mask >> 4;
        mask |= mask >> 8;
        mask |= mask >> 16;
        uint32_t v;
        while ((v = next32() & mask) > (uint32_t)mx) {
        }
        return (int)v;
    }
};

}  // namespace mgdp
