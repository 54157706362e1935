// vi_serve_depth.h -- the depth form of a served lone deterministic XYD grid (vi_serve_kernel,
// Loop::serve_pair, fresh requests): the solve from V_0 = +0 read off the goal depth of every state
// instead of swept.  Part of the single translation unit vi.hip (included from vi_loops.h, behind the
// served loops whose helpers it uses).  DESIGN.md §20 holds the proof and the measurements.
//
// The spec, in the working type T (terminal lava, no horizon, no slip, gamma >= 0, V_0 = +0):
//  * d(s): the breadth-first depth of state s = (cell, direction) searched backward from the goal; d = 1
//    for a valid state whose front cell is a goal; a state's successors are its two turns in place and,
//    where the front cell is walkable, the same direction in the front cell.
//  * g(1) = 1, g(n + 1) = fl(gamma * g(n)); g counts as +0 where a state has no depth.
//  * V_k[s] = g(d(s)) if d(s) <= k, else +0, bit for bit, for every k (fl and the multiplication by
//    gamma >= 0 are monotone, so the max over actions commutes with them; g does not increase, so a
//    state's first value is its last; the self loops give fl(gamma * V_k[s]) <= V_k[s] and never win).
//  * dV_k = g(k) if some state has depth k, else exactly 0.  With D the largest depth,
//    K = min(first k with dV_k < tol, max_sweeps): D + 1 if tol > 0, capped by the first k with
//    g(k) < tol and by max_sweeps.
//  * pi_K and V_K come from ONE real sweep on V_{K-1} (xyd_step, the per-action form the sweeping loops'
//    policy pass runs), so ties, gamma = 1 and the rounding of the last sweep need no argument.
//
// The layout.  Lane y of a wave holds row y of the grid as four W-bit reach masks, one per direction
// (W <= 32, H <= 64).  One level is, per direction, reach | the two turns | (reach of the front cell,
// shifted onto this cell) & walkable: the east / west shift is a bit shift in the lane, the north / south
// shift is the wave shift by one lane the served loops use for their east / west fronts (DPP wave_shl1 /
// wave_shr1, +0 shifted in).  No LDS read and no workgroup barrier lie on the per-level chain.  Wave 0
// alone searches (it holds thread 0, which publishes); the other waves wait at the request's one barrier.
// Levels go four at a time with no test between them; "no lane gained a bit" (one ballot) is asked of the
// fourth, and only the chunk in which the search ends asks it of the other three, from registers: the
// masks only grow, so the levels that gained are a prefix of the chunk.  Each level's four masks are
// stored, 16 bytes per row, into g_depth_lev (stores nobody waits for; lanes without a row store to a
// spare slot of their own, so the store needs no exec mask); a chunk may run up to three levels past the
// level the request needs, which the slots allow for and min(D, limit) discards.  K and dV are published
// as soon as D is known; {K, the levels to search, dV} then cross to the other waves through one LDS
// word behind an LDS-only barrier (a full one would wait for the publish's host stores).  Every cell
// thread then finds its six depths (its four states, plane 1 of the cell south of it and plane 3 of the
// cell north of it: the two fronts the last sweep reads that no DPP shift delivers) by binary search over
// the levels, all six in step: ceil(log2(min(D, K - 1) + 1)) rounds of six independent 4-byte LDS reads,
// then six reads of g.  This tail runs behind the publish, while the host turns the result around.
// Chosen over bit-sliced level counters (one direction per wave, every wave searching) by the
// instruction count on the request's path: one 16-byte store per level against 2 VALU per counter plane
// per level, and no assignment of directions to waves on workgroups of fewer than four.
//
// Limits, all handled inside the request by sweeping from V_0 (fused_serve_pair; path 2), never by
// refusing the grid: the levels that fit g_depth_lev (kDepthLevSlots / H - 4), the g table (kDepthTab)
// and MGDP_SERVE_DEPTH_MAX.  Grids wider than 32 or higher than 64, and grids whose wave edges keep them
// off the pair loop (serve_ew_ok), sweep as before (path 0).
//
// Kept per staged grid: the walkable and goal-front masks and each thread's (row, column).  Kept per
// launch of the server: g and the first k with g(k) < tol (gamma, tol and the dtype are the handle's).
// The search itself is redone in full for every request.
#pragma once

namespace mgdp {

constexpr int kDepthTab = 256;        // g(1..255); slot 0 holds the first k with g(k) < tol
constexpr int kDepthLevSlots = 2048;  // 16-byte slots of level masks: kDepthLevSlots / H levels
constexpr int kDepthChunk = 4;        // levels between two stop tests
constexpr int kDepthMaxW = 32, kDepthMaxH = 64;
constexpr int kDepthNever = 0x7fffffff;
constexpr int kDepthStaticLds = kDepthTab * 8 + (kDepthLevSlots + 64 + 1) * 16;  // bytes the arrays below add to the kernel
static __shared__ __attribute__((aligned(16))) unsigned long long g_depth_g[kDepthTab];
static __shared__ __attribute__((aligned(16))) uint4 g_depth_lev[kDepthLevSlots + 64];  // + a spare slot per lane
static __shared__ __attribute__((aligned(16))) uint4 g_depth_hand;  // wave 0 -> all: {K (0: abandoned), levels, dV bits}

// lane i <- lane i+1 / lane i-1 of the wave, 0 shifted in (dpp_shl1_zero / dpp_shr1_zero on a mask)
__device__ __forceinline__ uint32_t depth_row_below(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t depth_row_above(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}

// What the depth form keeps of a staged grid (resolved with the topology, once per grid).
struct ServeDepthTopo {
    uint32_t walk;   // lane = row: bit x = the agent may stand in cell (row, x)
    uint32_t gf[4];  // ... and, per direction, = it may and its front cell is a goal (depth 1)
    int y, x;        // this thread's cell; a thread without a cell sits on (H - 1, 0), a wall
    int ok;          // the grid takes the depth form (uniform)
};

// Once per launch, thread 0: g and the first k with g(k) < tol (kDepthNever if the table holds none).
// The caller's next barrier publishes them.
template <typename T>
__device__ __forceinline__ void serve_depth_table(const Coef<T> &cf) {
    if (threadIdx.x == 0) {
        T *g = reinterpret_cast<T *>(g_depth_g);
        int kt = kDepthNever;
        T v = (T)1;
        for (int n = 1; n < kDepthTab; ++n) {
            g[n] = v;
            if (kt == kDepthNever && v < cf.tol) kt = n;
            v = cf.g * v;
        }
        *reinterpret_cast<int *>(g_depth_g) = kt;  // g[0] is no table entry (g starts at 1): its bytes hold kt
    }
}
__device__ __forceinline__ int serve_depth_ktol() {
    return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int *>(g_depth_g));
}

// Whole workgroup, once per staged grid: the row masks from the cells in LDS (lane = row, in every wave).
__device__ __forceinline__ ServeDepthTopo serve_depth_topo(const uint8_t *cl, const Geo &geo, bool allowed) {
    ServeDepthTopo t;
    const int W = geo.W, H = geo.H, c = (int)threadIdx.x, row = c & 63;
    t.ok = allowed && W <= kDepthMaxW && H <= kDepthMaxH;
    t.y = c / W;
    t.x = c - t.y * W;
    if (c >= geo.HW) t.y = H - 1, t.x = 0;
    uint32_t walk = 0, gO = 0, gN = 0, gS = 0;
    if (t.ok && row < H) {
        for (int x = 0; x < W; ++x) {
            const uint32_t b = 1u << x;
            const int o = cl[row * W + x];
            if (xyd_free(o)) walk |= b;
            if (o == T_GOAL) gO |= b;
            if (row > 0 && cl[(row - 1) * W + x] == T_GOAL) gN |= b;
            if (row + 1 < H && cl[(row + 1) * W + x] == T_GOAL) gS |= b;
        }
    }
    t.walk = walk;
    t.gf[0] = walk & (gO >> 1);  // front of (y, x) facing east is (y, x + 1)
    t.gf[1] = walk & gS;
    t.gf[2] = walk & (gO << 1);
    t.gf[3] = walk & gN;
    return t;
}

#ifdef MGDP_SERVE_TRACE
// (stamp 0 also clears [4]: the host then knows the pair's split [1..4] is not this solve's)
#define MGDP_DEPTH_STAMP(i)                                           \
    do {                                                              \
        if (threadIdx.x == 0) {                                       \
            g_pair_trace[i] = __builtin_amdgcn_s_memtime();           \
            if ((i) == 0) g_pair_trace[4] = 0;                        \
        }                                                             \
    } while (0)
#else
#define MGDP_DEPTH_STAMP(i) do { } while (0)
#endif

// One fresh request.  Returns 1 with {k, dvl} published through `done` and V_K / pi_K stored, or 2 with
// nothing published, stored or changed but g_depth_lev: the caller then sweeps from V_0.
// lmax: MGDP_SERVE_DEPTH_MAX (the largest depth D the form searches out); ktol: serve_depth_ktol().
// Trace build: g_pair_trace[0] search start, [5] search end (the publish follows), [1] V and pi stores issued.
template <typename T, typename Done>
__device__ __forceinline__ int fused_serve_depth(const Geo &geo, const Coef<T> &cf, T *Vg_out, int8_t *pig, int &k,
                                                 double &dvl, const Done &done, const XydTopo<T> &tp,
                                                 const ServeDepthTopo &dt, int lmax, int ktol) {
    const int c = (int)threadIdx.x, lane = c & 63;
    const int H = geo.H;
    const bool own_cell = c < geo.HW;
    const T *g = reinterpret_cast<const T *>(g_depth_g);
    if (__builtin_amdgcn_readfirstlane(c >> 6) == 0) {  // wave 0 searches; the others wait at the barrier below
        // D <= lcap is searched out; level lcap + 1, if it exists, is only detected (and the request handed on).
        // A chunk may store kDepthChunk - 1 levels past `limit`: the slots allow for them.
        const int lcap = min(min(lmax, kDepthTab - 2), kDepthLevSlots / H - kDepthChunk);
        const int kcap = min(ktol, geo.max_sweeps);  // K <= kcap whatever the grid
        const int limit = min(kcap, lcap + 1);       // no level beyond it is needed
        MGDP_DEPTH_STAMP(0);
        uint32_t r0 = dt.gf[0], r1 = dt.gf[1], r2 = dt.gf[2], r3 = dt.gf[3];
        const uint32_t walk = dt.walk;
        // level l lives in slots (l - 1) * H ..; a lane without a row keeps storing to its spare slot
        const bool keeper = lane < H;
        uint4 *wp = keeper ? g_depth_lev + lane : g_depth_lev + kDepthLevSlots + lane;
        const int stride = keeper ? H : 0;
        auto gained = [](uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t b0, uint32_t b1, uint32_t b2,
                         uint32_t b3) -> int {
            uint32_t x = ((a0 ^ b0) | (a1 ^ b1)) | ((a2 ^ b2) | (a3 ^ b3));
            asm volatile("" : "+v"(x));  // one compare on the combined word, not one per mask
            return __ballot(x != 0u) != 0ull ? 1 : 0;
        };
        int D = 0;  // levels found so far (uniform)
        if (__ballot((r0 | r1 | r2 | r3) != 0u) != 0ull) {
            *wp = make_uint4(r0, r1, r2, r3);
            wp += stride;
            D = 1;
            while (D < limit) {
                uint32_t m[kDepthChunk + 1][4] = {{r0, r1, r2, r3}};
#pragma unroll
                for (int j = 1; j <= kDepthChunk; ++j) {
                    const uint32_t fS = depth_row_below(r1), fN = depth_row_above(r3);
                    const uint32_t t02 = r0 | r2, t13 = r1 | r3;
                    const uint32_t n0 = (r0 | t13 | (r0 >> 1)) & walk;
                    const uint32_t n1 = (r1 | t02 | fS) & walk;
                    const uint32_t n2 = (r2 | t13 | (r2 << 1)) & walk;
                    const uint32_t n3 = (r3 | t02 | fN) & walk;
                    r0 = n0, r1 = n1, r2 = n2, r3 = n3;
                    *wp = make_uint4(r0, r1, r2, r3);
                    wp += stride;
                    m[j][0] = r0, m[j][1] = r1, m[j][2] = r2, m[j][3] = r3;
                }
                auto gj = [&](int j) { return gained(m[j][0], m[j][1], m[j][2], m[j][3], m[j - 1][0], m[j - 1][1], m[j - 1][2], m[j - 1][3]); };
                if (gj(kDepthChunk)) {
                    D += kDepthChunk;
                    continue;
                }
                // the search ends in this chunk: the levels that gained are a prefix of it
#pragma unroll
                for (int j = 1; j < kDepthChunk; ++j) D += gj(j);
                break;
            }
        }
        D = min(D, limit);
        int K = 0;  // 0: abandoned
        T dv = (T)0;
        if (D <= lcap) {
            if (D == limit) {  // level kcap exists: the cap or the tolerance stops sweep kcap while states still change
                K = limit;
                dv = g[K];
            } else {  // sweep D + 1 changes nothing
                K = cf.tol > (T)0 ? D + 1 : geo.max_sweeps;
            }
            MGDP_DEPTH_STAMP(5);
            done(K, (double)dv);
        }
        if (lane == 0) {
            const unsigned long long b = (unsigned long long)__double_as_longlong((double)dv);
            g_depth_hand = make_uint4((unsigned)K, (unsigned)min(D, K - 1), (unsigned)b, (unsigned)(b >> 32));
        }
    }
    // wave 0's level stores and hand-over word; LDS only: __syncthreads would wait for the publish's host stores
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const uint4 hand = g_depth_hand;
    const int K = __builtin_amdgcn_readfirstlane((int)hand.x);
    if (K == 0) return 2;
    k = K;
    dvl = __longlong_as_double((long long)(((unsigned long long)__builtin_amdgcn_readfirstlane(hand.w) << 32) |
                                           (unsigned)__builtin_amdgcn_readfirstlane(hand.z)));
    // V_{K-1}: the first level of 1..Ls that holds the state (levels only grow), by binary search; pos = the
    // levels that do not.  Six states in step: this cell's four, (y + 1, x) facing south, (y - 1, x) facing north.
    const int Ls = __builtin_amdgcn_readfirstlane((int)hand.y);  // min(D, K - 1)
    const int top = Ls > 0 ? 1 << (31 - __builtin_clz((unsigned)Ls)) : 0;
    const int yS = min(dt.y + 1, H - 1), yN = max(dt.y - 1, 0);
    const uint32_t *const lw = reinterpret_cast<const uint32_t *>(g_depth_lev);
    const int base[6] = {dt.y * 4 + 0, dt.y * 4 + 1, dt.y * 4 + 2, dt.y * 4 + 3, yS * 4 + 1, yN * 4 + 3};
    const bool live[6] = {own_cell, own_cell, own_cell, own_cell, own_cell && dt.y + 1 < H, own_cell && dt.y >= 1};
    int pos[6] = {0, 0, 0, 0, 0, 0};
    for (int step = top; step > 0; step >>= 1) {  // uniform trip count
        uint32_t m[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) m[q] = lw[(min(pos[q] + step, Ls) - 1) * H * 4 + base[q]];
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (pos[q] + step <= Ls && ((m[q] >> dt.x) & 1u) == 0u) pos[q] += step;
    }
    T v[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = g[min(pos[q] + 1, Ls)];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = live[q] && pos[q] < Ls ? v[q] : (T)0;
    // the last sweep, for real: fused_serve_pair's policy pass on V_{K-1}; its output is V_K
    const T pE = dpp_shl1_zero(v[0]), pW = dpp_shr1_zero(v[2]);
    if (own_cell) {
        // (xyd_exit_pi_fronts<true> restated: through it vi_serve_kernel<T, XYD, serve_pair + depth> moved)
        const T geo_f[4] = {pE, v[4], pW, v[5]};
        const int HWs = geo.HWs;
        T nbv[4];
        V4<T> op;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            op.v[d] = v[d];
            nbv[d] = xyd_enters_soa(tp, d, c, HWs) ? geo_f[d] : v[d];
        }
        V4<T> vk;
        uint32_t pk;
        xyd_step<T, false, true>(tp, cf, op, nbv, vk, pk);
        *reinterpret_cast<uint32_t *>(pig + c * 4) = pk;
        *reinterpret_cast<V4<T> *>(Vg_out + c * 4) = vk;
    }
    MGDP_DEPTH_STAMP(1);
    return 1;
}

}  // namespace mgdp
