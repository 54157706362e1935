// envs.hip -- batched MiniGridEnv.step / gen_obs on MI355X (gfx950).
//
// Restates minigrid/minigrid_env.py:520-590 (step), :592-645 (gen_obs_grid / gen_obs),
// :448-479 (get_view_exts), :235-240 (_reward); minigrid/core/grid.py:110-143 (rotate_left,
// slice), :244-268 (encode), :291-328 (process_vis); minigrid/core/world_object.py (cell
// predicates, Door.toggle :185-195, Box.toggle :291-294).  Pinned by tests/test_gpu_step.py against
// 256-step trajectories captured from the reference (tests/golden/traj_*.npz) and against the
// oracle's step() restatement on 4096-env batches.
//
// Layout in HBM (B envs of W x H):
//   cell        uint8 [B][HWp]   one-byte cell code (type, colour, state), row-major, see cell_code
//   agent       int32 [B][4]     x, y, dir, step_count
//   carry       int32 [B][2]     carried (type, colour); type 0 = nothing
//   contents    uint8 [B][HWp]   optional (mgdp_envs_set_contents): the cell code of the object a
//                                Box at that cell holds (Box(contains=...), world_object.py:272-294),
//                                0 = none; ccontents uint8 [B]: the same for a carried Box
//   max_steps   int32 [B], see uint8 [B] (see_through_walls)
// One step = one envs_step_kernel launch: 2 lanes per env (see the kernel).  The V x V view is
// never materialised: view cell (i, j) maps to world top_left - f*j + r*i (f = DIR_TO_VEC[dir],
// r = right_vec, minigrid_env.py:421-446), which equals the reference's slice + (dir+1) x
// rotate_left; process_vis runs on a 64-bit visibility mask.
//
// Device code: the step kernel and the masked load's kernel here, envs_rollout.h (policy lookup, the
// fused rollout, the slip streams) and envs_qlearn.h (tabular Q-learning).  envs_codec.h (host-plain)
// is the cell code, the conversions between Grid.encode() layout and the planes, and the masked
// load's staging layout; timed.h the pooled event pairs of timed launches.  The host side: envs_host.h
// (the handle, launch_timed, the step launch, the grow-on-demand scratch), envs_host_state.h (load,
// get / set state, Box contents) and envs_host_episode.h (rollout, slip, explore, Q-learning: checks,
// kernel selection, host staging); this file holds the C ABI.
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_ext.h>

#include "common.h"
#include "envs_codec.h"
#include "pcg64.h"
#include "timed.h"

namespace mgdp {

__constant__ int kDX[4] = {1, 0, -1, 0};
__constant__ int kDY[4] = {0, 1, 0, -1};

struct EnvGeo {
    int B, W, H, HWp, vs;
    uint32_t nd_mask;   // NoDeath (wrappers.py:799-872): bit t = OBJECT_TO_IDX type t is a no-death type
    double death_cost;
};

// MGDP_STEP_NT: bit 0 = the obs tile leaves with nontemporal stores, bit 1 = the window rows are
// read with nontemporal loads (both streams are touched once per step; past the MALL at 2^20 envs)
#ifndef MGDP_STEP_NT
#define MGDP_STEP_NT 1  // measured: obs stores nt 92.3 -> 90.8 us (2^20 envs), 10.0 -> 9.3 us (65536); nt window loads 1.7x slower
#endif
__device__ __forceinline__ void copy_out(uint8_t *dst, const uint8_t *src, int bytes) {
    // dst is 16-B aligned: a workgroup's first env is a multiple of 32 (32*147 = 4704 = 16*294)
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (bytes & 15) == 0) {
        const uint4 *s = reinterpret_cast<const uint4 *>(src);
        uint4 *d = reinterpret_cast<uint4 *>(dst);
        for (int i = threadIdx.x; i < (bytes >> 4); i += blockDim.x) {
            if (MGDP_STEP_NT & 1) {
                const uint4 v = s[i];
                __builtin_nontemporal_store(v.x, &d[i].x);
                __builtin_nontemporal_store(v.y, &d[i].y);
                __builtin_nontemporal_store(v.z, &d[i].z);
                __builtin_nontemporal_store(v.w, &d[i].w);
            } else {
                d[i] = s[i];
            }
        }
    } else {
        for (int i = threadIdx.x; i < bytes; i += blockDim.x) dst[i] = src[i];
    }
}

// _reward: 1 - 0.9 * (step_count / max_steps), fp64, no contraction (minigrid_env.py:240)
__device__ __forceinline__ double reward_fn(int sc, int ms) {
    const double q = (double)sc / (double)ms;
    const double t = 0.9 * q;
    return 1.0 - t;
}

constexpr int kWinRow = 8;  // bytes per staged window row (vs + 1 <= 8 columns)

// The view's vs x vs cells always cover the axis-aligned world box [bx, bx+vs) x [by, by+vs)
// (rotation only permutes them); (tlx, tly) is the view's top-left (get_view_exts, :448-479).
__device__ __forceinline__ void view_box(int ax, int ay, int d, int vs, int &tlx, int &tly, int &bx, int &by) {
    const int hs = vs / 2;
    const int fx = kDX[d], fy = kDY[d], rx = -fy, ry = fx;
    tlx = ax + fx * (vs - 1) - rx * hs;
    tly = ay + fy * (vs - 1) - ry * hs;
    bx = tlx + min(0, -fx * (vs - 1)) + min(0, rx * (vs - 1));
    by = tly + min(0, -fy * (vs - 1)) + min(0, ry * (vs - 1));
}

// One env step: MiniGridEnv.step (minigrid_env.py:520-590) on registers; the front-cell mutation
// of pickup / drop / toggle is returned (mut, nt/nc/ns) instead of written, so the caller orders it
// against the window it stages.
struct StepOut {
    int x, y, d, sc, ct, cc, stat, term, trunc, mut, fi, nt, nc, ns, op;  // op: kOp* (front-cell action)
    double r;
};
enum { kOpNone = 0, kOpPickup = 1, kOpDrop = 2, kOpToggleBox = 3 };

// Rd: cell reader, rd(x, y) -> (type, colour, state) of in-grid cell (x, y) of this env.
template <typename Rd>
__device__ __forceinline__ StepOut step_core(const EnvGeo &g, const Rd &rd, int x, int y, int d, int sc, int ct,
                                             int cc, int a, int ms) {
    // Branch-free over the action (a wave steps envs with different actions): every effect is
    // computed and selected.  step_count += 1 first (:523); an out-of-grid front cell fails before
    // the action branch (Grid.get assert, :533), an unknown action after it (:579-580).
    StepOut o{x, y, d, sc + 1, ct, cc, MGDP_OK, 0, 0, 0, 0, 0, 0, 0, kOpNone, 0.0};
    const int fx = x + kDX[d], fy = y + kDY[d];
    const bool inb = (unsigned)fx < (unsigned)g.W && (unsigned)fy < (unsigned)g.H;
    const bool act_ok = (unsigned)a <= 6u;
    o.stat = !inb ? MGDP_E_BOUNDS : !act_ok ? MGDP_E_ACTION : MGDP_OK;
    const int fi = inb ? fy * g.W + fx : 0;
    int ft, fc, fs;
    rd(inb ? fx : 0, inb ? fy : 0, ft, fc, fs);
    const bool ok = o.stat == MGDP_OK;
    const bool fnone = ft == T_EMPTY;
    // left / right (:536-541)
    o.d = !ok ? d : a == 0 ? ((d + 3) & 3) : a == 1 ? ((d + 1) & 3) : d;
    // forward (:544-553): can_overlap = Goal, Floor, Lava, open Door (world_object.py)
    const bool fwd = ok && a == 2;
    const uint32_t fb = 1u << (ft & 31);  // type bit: comparison chains are lowered to branches
    const bool overlap = ((fb & ((1u << T_GOAL) | (1u << T_FLOOR) | (1u << T_LAVA))) != 0) | ((ft == T_DOOR) & (fs == D_OPEN));
    const bool move = fwd && (fnone || overlap);
    o.x = move ? fx : x;
    o.y = move ? fy : y;
    const bool goal = fwd && ft == T_GOAL;
    o.term = goal || (fwd && ft == T_LAVA);
    if (goal) o.r = reward_fn(o.sc, ms);
    // pickup (:556-561): Key / Ball / Box, hands empty
    const bool pickup = ok & (a == 3) & ((fb & ((1u << T_KEY) | (1u << T_BALL) | (1u << T_BOX))) != 0) & (ct == 0);
    // drop (:564-568): front empty, carrying
    const bool drop = ok && a == 4 && fnone && ct != 0;
    // toggle (:571-575): Door.toggle (locked: needs the carried Key of its colour, unlocks and
    // opens; else flips is_open, world_object.py:185-195); Box.toggle -> its contents (:291-294):
    // empty here, the caller puts a held object from the contents plane in its place
    const bool tdoor = ok && a == 5 && ft == T_DOOR && (fs != D_LOCKED || (ct == T_KEY && cc == fc));
    const bool tbox = ok && a == 5 && ft == T_BOX;
    const bool clear = pickup || tbox;
    o.mut = clear || drop || tdoor;
    o.op = pickup ? kOpPickup : drop ? kOpDrop : tbox ? kOpToggleBox : kOpNone;
    o.fi = fi;
    o.nt = clear ? T_EMPTY : drop ? ct : ft;
    o.nc = clear ? 0 : drop ? cc : fc;
    o.ns = tdoor ? (fs == D_OPEN ? D_CLOSED : D_OPEN) : 0;
    o.ct = pickup ? ft : drop ? 0 : ct;
    o.cc = pickup ? fc : drop ? 0 : cc;
    if (!ok) return o;
    if (o.sc >= ms) o.trunc = 1;
    if (g.nd_mask) {  // NoDeath.step: front cell before, agent's cell after the step (never mutated)
        const bool going = a == 2 && !fnone && ((g.nd_mask >> ft) & 1u);
        int ct_now, c_now, s_now;
        rd(o.x, o.y, ct_now, c_now, s_now);
        const bool in_death = ct_now != T_EMPTY && ((g.nd_mask >> ct_now) & 1u);
        if (o.term && (going || in_death)) {
            o.term = 0;
            o.r += g.death_cost;
        }
    }
    return o;
}

// ------------------------------------------------------------------------------------------------
// envs_step_kernel: G = 2 (or 1, 4, 8: MGDP_STEP_GROUP) lanes per env, 256 / G envs per 256-thread
// workgroup, so a 65536-env batch is 2048 waves (2 per SIMD).  Per env:
//   * lane v stages row v of the window box with 3 dword loads aligned by v_alignbyte into the
//     group's LDS window.  The box is the view box after the turn (left / right change only the
//     direction), extended by one cell along the heading for forward, so it holds both possible
//     views, the front cell and the agent's next cell: one dependent HBM round trip after the
//     agent record, and the step reads LDS.  The wave executes its LDS accesses in issue order, so
//     the other lanes' rows are visible without a barrier (the group lies inside one wave);
//   * every lane runs step_core on the window (uniform per group); lane 0 alone writes the per-env
//     results and the front-cell mutation (window and HBM);
//   * lane i < vs owns view column i: its see-behind bits are OR-reduced over the group (xor
//     shuffles), process_vis runs on the 64-bit mask in bit-parallel form (process_vis_bits), and
//     the lane encodes its column -- obs bytes [3*vs*i, 3*vs*(i+1)) of the env, contiguous because
//     the obs is x-major -- into the LDS obs tile, which leaves with 16-B coalesced stores.
// Measured (DoorKey-16 x 65536 per step, profiles/r01_step/): one thread per env on three byte
// planes 49 us; 8 lanes per env 16.5 us; one byte plane + one round trip 15.7 us; 4 lanes 11.4 us;
// out-of-grid cells staged as walls + a code -> (encoding, see_behind) table in LDS: 4 lanes
// 11.1 us, 2 lanes 10.2 us.
// ------------------------------------------------------------------------------------------------
constexpr int kGroupBlock = 256;  // threads per workgroup (G lanes per env, 256 / G envs)

__device__ __forceinline__ uint32_t rev8(uint32_t v) { return __builtin_bitreverse32(v) >> 24; }

// process_vis (grid.py:291-328) on the see-behind mask sb (bit j*8+i = view cell (i, j)), one row
// per step from j = vs-1 up.  In row j the left-to-right pass visits i = 0..vs-2: a visible
// see-behind cell makes i+1 visible and marks (i, j-1), (i+1, j-1).  Bit i's value when visited is
// final for that pass (only i-1 can set it before), so the pass equals the closure of the row's
// seeds m moving up through the see-behind run p = sb & [0, vs-2]: adding the seeds x = m & p to p
// carries through each seeded run and sets the bit past its end, hence L = m | ((p + x) ^ p).  The
// right-to-left pass (i = vs-1..1) is the same closure in bit-reversed order, seeded by L.  Checked
// against the literal loop on 200k random masks for vs = 3, 5, 7 before use.
template <int VS>
__device__ __forceinline__ unsigned long long process_vis_bits(unsigned long long sb) {
    constexpr uint32_t limL = (1u << (VS - 1)) - 1u;
    constexpr uint32_t limR = ((1u << VS) - 1u) & ~1u;
    unsigned long long mask = 0;
    uint32_t up = 0;
#pragma unroll
    for (int j = VS - 1; j >= 0; --j) {
        const uint32_t m = up | (j == VS - 1 ? 1u << (VS / 2) : 0u);
        const uint32_t s = (uint32_t)(sb >> (8 * j)) & 0xffu;
        const uint32_t p = s & limL;
        const uint32_t L = m | ((p + (m & p)) ^ p);
        const uint32_t g1 = L & p;
        const uint32_t q = s & limR;
        const uint32_t Lr = rev8(L), qr = rev8(q);
        const uint32_t R = rev8(Lr | ((qr + (Lr & qr)) ^ qr));
        const uint32_t g2 = R & q;
        up = g1 | (g1 << 1) | g2 | (g2 >> 1);
        mask |= (unsigned long long)R << (8 * j);
    }
    return mask;
}

template <int G>
__device__ __forceinline__ unsigned long long group_or(unsigned long long v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, o);
        hi |= (uint32_t)__shfl_xor((int)hi, o);
    }
    return ((unsigned long long)hi << 32) | lo;
}

template <int VS, int G>
__global__ void __launch_bounds__(kGroupBlock)
envs_step_kernel(EnvGeo g, uint8_t *__restrict__ CELL, int32_t *__restrict__ agent, int32_t *__restrict__ carry,
                 uint8_t *__restrict__ cont, uint8_t *__restrict__ ccont, const int32_t *__restrict__ max_steps, const uint8_t *__restrict__ see,
                 const int32_t *__restrict__ actions, uint8_t *__restrict__ obs,
                 int32_t *__restrict__ direction, double *__restrict__ reward,
                 uint8_t *__restrict__ terminated, uint8_t *__restrict__ truncated,
                 int32_t *__restrict__ status, int observe_only) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int OB = VS * VS * 3;  // obs bytes per env
    constexpr int WR = VS + 1;       // staged rows: the view box plus the forward cell
    constexpr int RB = kWinRow;
    constexpr int WD = WR * RB / 4;  // window dwords per env
    constexpr int NE = kGroupBlock / G;        // envs per workgroup
    constexpr int NR = (WR + G - 1) / G;       // window rows staged per lane
    constexpr int NC = (VS + G - 1) / G;       // view columns per lane
    const int slot = threadIdx.x / G, r = threadIdx.x % G;
    const int e0 = blockIdx.x * NE;
    const int e = e0 + slot;
    uint8_t *img = smem + slot * OB;
    uint32_t *win = reinterpret_cast<uint32_t *>(smem + round_up(NE * OB, 16)) + slot * (WD + 1);
    uint8_t *wb = reinterpret_cast<uint8_t *>(win);
    // cell code -> encoded (type | colour << 8 | state << 16) | see_behind << 24 (world_object.py:
    // not a wall, not a closed / locked door); read per view cell instead of decoding
    __shared__ uint32_t lut[256];
    {
        int t, c, st;
        cell_decode(threadIdx.x, t, c, st);  // blockDim == 256: one entry per thread
        c = t == T_EMPTY ? 0 : c;
        const bool behind = t != T_WALL && !(t == T_DOOR && st != D_OPEN);
        lut[threadIdx.x] = (uint32_t)t | ((uint32_t)c << 8) | ((uint32_t)st << 16) | ((uint32_t)behind << 24);
    }
    __syncthreads();
    if (e < g.B) {
        uint8_t *cell = CELL + (long long)e * g.HWp;
        const int4 ag = reinterpret_cast<const int4 *>(agent)[e];
        const int2 cr = reinterpret_cast<const int2 *>(carry)[e];
        const int act = observe_only ? -1 : actions[e];
        const int ms = observe_only ? 1 : max_steps[e];
        const int d1 = act == 0 ? ((ag.z + 3) & 3) : act == 1 ? ((ag.z + 1) & 3) : ag.z;
        int tlx, tly, bx, by;
        view_box(ag.x, ag.y, d1, VS, tlx, tly, bx, by);
        if (act == 2) { bx += min(kDX[ag.z], 0); by += min(kDY[ag.z], 0); }
#pragma unroll
        for (int k = 0; k < NR; ++k) {  // lane r stages window rows r, r+G, ...
            const int row = r + G * k;
            if (row < WR) {
                const int nd = g.HWp >> 2;
                const int off = (by + row) * g.W + bx;
                const int a = off >> 2;  // floor: off may be negative left of / above the grid
                const int sh = off & 3;
                const uint32_t *P = reinterpret_cast<const uint32_t *>(cell);
                uint32_t w[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {  // clamped: out-of-grid bytes are replaced below
                    const uint32_t *pq = P + min(max(a + q, 0), nd - 1);
                    w[q] = (MGDP_STEP_NT & 2) ? __builtin_nontemporal_load(pq) : *pq;
                }
                // Out-of-grid cells of the window become grey walls: slice() fills them with Wall()
                // (grid.py:136-139), which encodes and blocks sight exactly like a grid wall, so the
                // view loops below need no bounds tests.  Bytes [lo, hi) of the row are in the grid.
                const int y = by + row;
                const int lo = min(max(-bx, 0), 8), hi = (unsigned)y < (unsigned)g.H ? min(max(g.W - bx, 0), 8) : 0;
                const unsigned long long keep = (hi > lo ? (~0ull >> (64 - 8 * (hi - lo))) << (8 * lo) : 0ull);
                const unsigned long long bytes = ((unsigned long long)__builtin_amdgcn_alignbyte(w[2], w[1], sh) << 32) |
                                                 __builtin_amdgcn_alignbyte(w[1], w[0], sh);
                const unsigned long long v = (bytes & keep) | (0x0101010101010101ull * kCodeWall & ~keep);
                win[row * 2 + 0] = (uint32_t)v;
                win[row * 2 + 1] = (uint32_t)(v >> 32);
            }
        }
        asm volatile("" ::: "memory");  // the group's rows are written before any lane reads them
        StepOut o{ag.x, ag.y, ag.z, ag.w, cr.x, cr.y, MGDP_OK, 0, 0, 0, 0, 0, 0, 0, kOpNone, 0.0};
        if (!observe_only) {
            // cells outside the staged box are only asked for by turns (whose result ignores them)
            const auto rd = [&](int cx, int cy, int &t, int &c, int &s) {
                const int u = cx - bx, v = cy - by;
                const bool in = (unsigned)u < (unsigned)RB && (unsigned)v < (unsigned)WR;
                cell_decode(in ? wb[v * RB + u] : 0u, t, c, s);
            };
            o = step_core(g, rd, ag.x, ag.y, ag.z, ag.w, cr.x, cr.y, act, ms);
        }
        if (o.stat == MGDP_OK) {
            int bx2, by2;
            view_box(o.x, o.y, o.d, VS, tlx, tly, bx2, by2);
            asm volatile("" ::: "memory");
            if (o.mut && r == 0) {  // the front cell as the step left it (in the view: the agent did not move)
                const int fy = o.fi / g.W, fx = o.fi - fy * g.W;
                uint8_t code = (uint8_t)cell_code(o.nt, o.nc, o.ns);
                if (cont) {  // contents plane present (a uniform test): what Boxes hold moves with them
                    uint8_t *cf = cont + (long long)e * g.HWp + o.fi;
                    if (o.op == kOpToggleBox) {  // the box is replaced by what it held (None: empty)
                        const uint8_t held = *cf;
                        code = held ? held : code;
                        *cf = 0;
                    } else if (o.op == kOpPickup) {  // a carried Box keeps its contents
                        ccont[e] = *cf;
                        *cf = 0;
                    } else if (o.op == kOpDrop) {
                        *cf = ccont[e];
                        ccont[e] = 0;
                    }
                }
                wb[(fy - by) * RB + (fx - bx)] = code;
                cell[o.fi] = code;
            }
            asm volatile("" ::: "memory");
            const int fx = kDX[o.d], fy = kDY[o.d], rx = -fy, ry = fx;
            // Lane r owns view columns i = r, r+G, ...  View cell (i, j) is world (wx0 - fx*j,
            // wy0 - fy*j) with wx0 = tlx + rx*i, wy0 = tly + ry*i: window byte ow0 - j*(8*fy + fx).
            // Every view cell lies in the staged box, and out-of-grid ones hold wall codes.
            const int dj = RB * fy + fx;
            uint32_t cv[NC][VS];
            unsigned long long sb = 0;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int i = min(r + G * k, VS - 1);  // lanes past the view re-read column VS-1, contribute no bits
                const int ow0 = (tly + ry * i - by) * RB + (tlx + rx * i - bx);
#pragma unroll
                for (int j = 0; j < VS; ++j) {
                    cv[k][j] = lut[wb[ow0 - j * dj]];
                    if (r + G * k < VS) sb |= (unsigned long long)(cv[k][j] >> 24) << (j * 8 + i);
                }
            }
            sb = group_or<G>(sb);
            const unsigned long long mask = see[e] ? ~0ull : process_vis_bits<VS>(sb);
            const uint32_t carried = o.ct > 0 ? (uint32_t)o.ct | ((uint32_t)o.cc << 8) : (uint32_t)T_EMPTY;
#pragma unroll
            for (int k = 0; k < NC; ++k) {  // encode column i, grid.py:244-268; the carried object at (VS/2, VS-1)
                const int i = r + G * k;
                if (i < VS) {
                    uint8_t *col = img + i * VS * 3;
#pragma unroll
                    for (int j = 0; j < VS; ++j) {
                        uint32_t x = (j == VS - 1 && i == VS / 2) ? carried : cv[k][j];
                        x = (mask >> (j * 8 + i)) & 1ull ? x : 0u;
                        col[3 * j] = (uint8_t)x;
                        col[3 * j + 1] = (uint8_t)(x >> 8);
                        col[3 * j + 2] = (uint8_t)(x >> 16);
                    }
                }
            }
        } else {
            for (int k = r; k < OB; k += G) img[k] = 0;
        }
        if (r == 0) {
            if (!observe_only) {
                reinterpret_cast<int4 *>(agent)[e] = make_int4(o.x, o.y, o.d, o.sc);
                reinterpret_cast<int2 *>(carry)[e] = make_int2(o.ct, o.cc);
                reward[e] = o.r;
                terminated[e] = (uint8_t)o.term;
                truncated[e] = (uint8_t)o.trunc;
                status[e] = o.stat;
            }
            direction[e] = o.d;
        }
    }
    __syncthreads();
    const int n = min(NE, g.B - e0);
    copy_out(obs + (long long)e0 * OB, smem, n * OB);
}

#include "envs_rollout.h"  // tabular policies on resident envs: policy lookup and the fused rollout
#include "envs_qlearn.h"   // tabular Q-learning on resident envs, episode restarts inside the launch

// A masked reset (state_load, envs_host_state.h): one block per env writes a masked env's cells, agent,
// carry, max_steps and see_through from the staging buffer st (StageLayout, envs_codec.h) and clears its
// Box contents.
extern "C" __global__ void __launch_bounds__(64)
envs_masked_load_kernel(int B, int HWp, const uint8_t *__restrict__ st, uint8_t *__restrict__ cell, int32_t *__restrict__ agent,
                        int32_t *__restrict__ carry, int32_t *__restrict__ maxs, uint8_t *__restrict__ see,
                        uint8_t *__restrict__ cont, uint8_t *__restrict__ ccont) {
    const int b = blockIdx.x;
    const StageLayout L{B, HWp};
    if (!st[L.mask(b)]) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(L.cells(st) + (size_t)b * HWp);
    uint4 *dst = reinterpret_cast<uint4 *>(cell + (size_t)b * HWp);
    for (int i = threadIdx.x; i < HWp / 16; i += blockDim.x) {
        dst[i] = src[i];
        if (cont) reinterpret_cast<uint4 *>(cont + (size_t)b * HWp)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (threadIdx.x == 0) {
        const int32_t *ag = L.agent(st), *cr = L.carry(st), *ms = L.max(st);
        for (int j = 0; j < 4; ++j) agent[4 * b + j] = ag[4 * b + j];
        carry[2 * b] = cr[2 * b];
        carry[2 * b + 1] = cr[2 * b + 1];
        maxs[b] = ms[b];
        see[b] = st[L.see(b)];
        if (ccont) ccont[b] = 0;
    }
}

}  // namespace mgdp

// ================================================================================================
// Host side
// ================================================================================================
using namespace mgdp;

#include "envs_host.h"
#include "envs_host_state.h"
#include "envs_host_episode.h"

extern "C" {

int mgdp_envs_create(int32_t device, int32_t B, int32_t W, int32_t H, int32_t view_size, mgdp_envs **out) {
    MGDP_CHECK(out, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(B > 0 && W >= 3 && H >= 3, MGDP_E_INVALID, "bad shape B=%d W=%d H=%d", B, W, H);
    MGDP_CHECK(view_size >= 3 && view_size <= 7 && (view_size & 1), MGDP_E_INVALID,
               "agent_view_size must be odd and in [3, 7] (got %d)", view_size);
    int ndev = 0;
    MGDP_HIP(hipGetDeviceCount(&ndev));
    MGDP_CHECK(device >= 0 && device < ndev, MGDP_E_HIP, "device %d not available (%d visible)", device, ndev);
    int group = 2;
    if (const char *ev = std::getenv("MGDP_STEP_GROUP")) {
        group = std::atoi(ev);
        MGDP_CHECK(group == 1 || group == 2 || group == 4 || group == 8, MGDP_E_INVALID,
                   "MGDP_STEP_GROUP must be 1, 2, 4 or 8 (got %s)", ev);
    }
    int roll_reader = -1;
    if (const char *ev = std::getenv("MGDP_ROLLOUT_READER")) {  // A/B of the rollout's cell reader (tools/probe_rollout.py)
        roll_reader = !std::strcmp(ev, "hbm") ? 0 : !std::strcmp(ev, "lds") ? 1 : -2;
        MGDP_CHECK(roll_reader != -2, MGDP_E_INVALID, "MGDP_ROLLOUT_READER must be hbm or lds (got %s)", ev);
    }
    DeviceGuard guard(device);
    MGDP_CHECK(guard.ok, MGDP_E_HIP, "hipSetDevice(%d) failed", device);
    mgdp_envs *E = new mgdp_envs();
    E->group = group;
    E->roll_reader = roll_reader;
    E->device = device; E->B = B; E->W = W; E->H = H; E->HW = W * H; E->HWp = (int)round_up(W * H, 16);
    E->vs = view_size;
    const size_t P = (size_t)B * E->HWp;
    hipError_t e = hipSuccess;
    auto al = [&](void **p, size_t n) { if (e == hipSuccess) e = hipMalloc(p, n); };
    al((void **)&E->d_cell, P);
    al((void **)&E->d_see, B);
    al((void **)&E->d_agent, sizeof(int32_t) * 4 * B);
    al((void **)&E->d_carry, sizeof(int32_t) * 2 * B);
    al((void **)&E->d_max, sizeof(int32_t) * B);
    al((void **)&E->d_act, sizeof(int32_t) * B);
    al((void **)&E->d_dir, sizeof(int32_t) * B);
    al((void **)&E->d_status, sizeof(int32_t) * B);
    al((void **)&E->d_obs, (size_t)B * view_size * view_size * 3);
    al((void **)&E->d_term, B); al((void **)&E->d_trunc, B);
    al((void **)&E->d_rew, sizeof(double) * B);
    if (e == hipSuccess) { e = hipStreamCreateWithFlags(&E->stream, hipStreamNonBlocking); E->own_stream = e == hipSuccess; }
    if (e == hipSuccess) e = hipMemset(E->d_cell, (int)kCodeWall, P);
    if (e == hipSuccess) e = hipMemset(E->d_agent, 0, sizeof(int32_t) * 4 * B);
    if (e == hipSuccess) e = hipMemset(E->d_carry, 0, sizeof(int32_t) * 2 * B);
    if (e != hipSuccess) {
        mgdp_envs_destroy(E);
        return hip_fail(e, "mgdp_envs_create allocation", __FILE__, __LINE__);
    }
    *out = E;
    return 0;
}

int mgdp_envs_destroy(mgdp_envs *E) {
    if (!E) return 0;
    DeviceGuard guard(E->device);
    if (E->stream) (void)hipStreamSynchronize(E->stream);
    void *ps[] = {E->d_cell, E->d_see, E->d_agent, E->d_carry, E->d_max, E->d_act,
                  E->d_dir, E->d_status, E->d_obs, E->d_term, E->d_trunc, E->d_rew, E->d_cont, E->d_ccont, E->stage.p,
                  E->roll.p, E->slip.state, E->slip.half, E->explore.state, E->explore.half, E->d_stream_mask};
    for (void *p : ps) (void)hipFree(p);
    E->timed.destroy();
    if (E->own_stream) (void)hipStreamDestroy(E->stream);
    delete E;
    return 0;
}

int mgdp_envs_set_nodeath(mgdp_envs *E, uint32_t type_mask, double death_cost) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(!(type_mask & (1u << T_GOAL)), MGDP_E_INVALID, "goal cannot be a death cell (wrappers.py:845)");
    MGDP_CHECK(!(type_mask & (1u << T_EMPTY)), MGDP_E_INVALID, "an empty cell is no object");
    E->nd_mask = type_mask;
    E->death_cost = death_cost;
    return 0;
}

int mgdp_envs_set_stream(mgdp_envs *E, void *s) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    MGDP_HIP(hipStreamSynchronize(E->stream));
    if (E->own_stream) { (void)hipStreamDestroy(E->stream); E->own_stream = false; E->stream = nullptr; }
    if (s) E->stream = (hipStream_t)s;
    else { MGDP_HIP(hipStreamCreateWithFlags(&E->stream, hipStreamNonBlocking)); E->own_stream = true; }
    return 0;
}

int mgdp_envs_load(mgdp_envs *E, const uint8_t *enc, const int32_t *agent, const int32_t *max_steps,
                   const uint8_t *see_through, const uint8_t *mask) {
    MGDP_CHECK(E && enc && agent && max_steps && see_through, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return state_load(E, enc, agent, max_steps, see_through, mask);
}

int mgdp_envs_observe(mgdp_envs *E, uint8_t *obs, int32_t *direction) {
    MGDP_CHECK(E && obs, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    if (int rc = launch_step(E, nullptr, E->d_obs, E->d_dir, E->d_rew, E->d_term, E->d_trunc, E->d_status, 1)) return rc;
    const size_t ob = (size_t)E->B * E->vs * E->vs * 3;
    MGDP_HIP(hipMemcpyAsync(obs, E->d_obs, ob, hipMemcpyDeviceToHost, E->stream));
    if (direction) MGDP_HIP(hipMemcpyAsync(direction, E->d_dir, 4 * (size_t)E->B, hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

int mgdp_envs_step_device(mgdp_envs *E, const int32_t *d_actions, uint8_t *d_obs, int32_t *d_direction,
                          double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, int32_t *d_status) {
    MGDP_CHECK(E && d_actions && d_obs && d_direction && d_reward && d_terminated && d_truncated && d_status,
               MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return launch_step(E, d_actions, d_obs, d_direction, d_reward, d_terminated, d_truncated, d_status, 0);
}

int mgdp_envs_step(mgdp_envs *E, const int32_t *actions, uint8_t *obs, int32_t *direction, double *reward,
                   uint8_t *terminated, uint8_t *truncated, int32_t *status) {
    MGDP_CHECK(E && actions, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    const size_t B = E->B;
    MGDP_HIP(hipMemcpyAsync(E->d_act, actions, 4 * B, hipMemcpyHostToDevice, E->stream));
    if (int rc = launch_step(E, E->d_act, E->d_obs, E->d_dir, E->d_rew, E->d_term, E->d_trunc, E->d_status, 0)) return rc;
    std::vector<int32_t> st_local;
    int32_t *stat = status;
    if (!stat) { st_local.resize(B); stat = st_local.data(); }
    if (download(E, obs, E->d_obs, B * E->vs * E->vs * 3) || download(E, direction, E->d_dir, 4 * B) ||
        download(E, reward, E->d_rew, 8 * B) || download(E, terminated, E->d_term, B) ||
        download(E, truncated, E->d_trunc, B) || download(E, stat, E->d_status, 4 * B))
        return MGDP_E_HIP;
    MGDP_HIP(hipStreamSynchronize(E->stream));
    for (size_t b = 0; b < B; ++b) {
        if (stat[b] == MGDP_E_ACTION) { set_error("Unknown action: %d (env %zu)", actions[b], b); return MGDP_E_ACTION; }
        if (stat[b] == MGDP_E_BOUNDS) { set_error("env %zu: front cell outside the grid", b); return MGDP_E_BOUNDS; }
    }
    return 0;
}

int mgdp_envs_enable_timing(mgdp_envs *E, int32_t on) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return E->timed.restart(on != 0);  // drops launches timed before this call
}

int mgdp_envs_kernel_time(mgdp_envs *E, double *total_ms, int64_t *launches) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return E->timed.read(total_ms, launches);
}

int mgdp_envs_get_state(mgdp_envs *E, uint8_t *enc, int32_t *agent, int32_t *carry, int32_t *step_count) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    return state_get(E, enc, agent, carry, step_count);
}

int mgdp_envs_set_state(mgdp_envs *E, const int32_t *agent, const int32_t *carry, const int32_t *step_count,
                        const uint8_t *mask) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    return state_set(E, agent, carry, step_count, mask);
}

int mgdp_envs_set_contents(mgdp_envs *E, const uint8_t *contents, const int32_t *carry_contents) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    return contents_set(E, contents, carry_contents);
}

int mgdp_envs_get_contents(mgdp_envs *E, uint8_t *contents, int32_t *carry_contents) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    DeviceGuard guard(E->device);
    return contents_get(E, contents, carry_contents);
}

// ---- policy lookup and fused rollout ---------------------------------------
int mgdp_envs_policy_actions_device(mgdp_envs *E, int32_t model, const int8_t *d_pi, int32_t T, int32_t *d_actions,
                                    int32_t *d_status) {
    int S = 0;
    if (int rc = roll_check(E, model, d_pi, T, &S)) return rc;
    MGDP_CHECK(d_actions && d_status, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return launch_policy_actions(E, model, d_pi, T, S, d_actions, d_status);
}

int mgdp_envs_rollout_device(mgdp_envs *E, int32_t model, const int8_t *d_pi, int32_t T, int32_t n_max, int32_t *d_steps,
                             double *d_ret, uint8_t *d_terminated, uint8_t *d_truncated, int32_t *d_status,
                             int32_t *d_trace_state, int8_t *d_trace_action, int32_t trace_len) {
    int S = 0;
    if (int rc = roll_check(E, model, d_pi, T, &S)) return rc;
    MGDP_CHECK(d_steps && d_ret && d_terminated && d_truncated && d_status, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(trace_len >= 0, MGDP_E_INVALID, "trace_len must be >= 0, got %d", trace_len);
    TraceBufs t;
    if (int rc = trace_device(d_trace_state, d_trace_action, trace_len, &t)) return rc;
    DeviceGuard guard(E->device);
    const RolloutArgs r{d_pi, T, S, n_max, t.len, d_steps, d_ret, d_terminated, d_truncated, d_status, t.state, t.act};
    return launch_rollout(E, model, r);
}

int mgdp_envs_policy_actions(mgdp_envs *E, int32_t model, const int8_t *pi, int32_t T, int32_t *actions, int32_t *status) {
    int S = 0;
    if (int rc = roll_check(E, model, pi, T, &S)) return rc;
    MGDP_CHECK(actions, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return policy_actions_host(E, model, pi, T, S, actions, status);
}

int mgdp_envs_rollout(mgdp_envs *E, int32_t model, const int8_t *pi, int32_t T, int32_t n_max, int32_t *steps, double *ret,
                      uint8_t *terminated, uint8_t *truncated, int32_t *status, int32_t *trace_state,
                      int8_t *trace_action, int32_t trace_len) {
    int S = 0;
    if (int rc = roll_check(E, model, pi, T, &S)) return rc;
    MGDP_CHECK(trace_len >= 0, MGDP_E_INVALID, "trace_len must be >= 0, got %d", trace_len);
    TraceBufs h;  // the caller's buffers; none: no trace is taken
    if (int rc = trace_host(trace_state, trace_action, trace_len, &h)) return rc;
    DeviceGuard guard(E->device);
    return rollout_host(E, model, pi, T, S, n_max, steps, ret, terminated, truncated, status, h);
}

// ---- slip: per-env PCG64 action noise ---------------------------------------
int mgdp_envs_set_slip(mgdp_envs *E, double prob, int32_t random_action, uint64_t seed0, const uint8_t *mask) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(prob >= 0.0 && prob <= 1.0, MGDP_E_INVALID, "slip prob must be in [0, 1], got %g", prob);  // NaN fails both
    MGDP_CHECK(random_action >= -1 && random_action <= 6, MGDP_E_INVALID,
               "random_action must be an env action 0..6 or -1 (draw one of 0..5), got %d", random_action);
    if (int rc = seed_streams(E, E->slip, seed0, mask, "mgdp_envs_set_slip")) return rc;
    E->slip_p = prob;
    E->slip_ra = random_action;
    return 0;
}

int mgdp_envs_clear_slip(mgdp_envs *E) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    E->slip.on = false;  // the records stay allocated; the next set_slip is a first call again
    return 0;
}

int mgdp_envs_get_slip_streams(mgdp_envs *E, uint64_t *state, uint32_t *half) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(E->slip.on, MGDP_E_INVALID, "no slip set on this handle (mgdp_envs_set_slip)");
    return read_streams(E, E->slip, state, half);
}

int mgdp_envs_slip_actions_device(mgdp_envs *E, const int32_t *d_in, int32_t *d_out) {
    MGDP_CHECK(E && d_in && d_out, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(E->slip.on, MGDP_E_INVALID, "no slip set on this handle (mgdp_envs_set_slip)");
    DeviceGuard guard(E->device);
    return launch_slip_actions(E, d_in, d_out);
}

int mgdp_envs_slip_actions(mgdp_envs *E, const int32_t *in, int32_t *out) {
    MGDP_CHECK(E && in && out, MGDP_E_INVALID, "null argument");
    MGDP_CHECK(E->slip.on, MGDP_E_INVALID, "no slip set on this handle (mgdp_envs_set_slip)");
    DeviceGuard guard(E->device);
    const size_t B = E->B;
    MGDP_HIP(hipMemcpyAsync(E->d_act, in, 4 * B, hipMemcpyHostToDevice, E->stream));
    if (int rc = launch_slip_actions(E, E->d_act, E->d_act)) return rc;
    MGDP_HIP(hipMemcpyAsync(out, E->d_act, 4 * B, hipMemcpyDeviceToHost, E->stream));
    MGDP_HIP(hipStreamSynchronize(E->stream));
    return 0;
}

// ---- tabular Q-learning ------------------------------------------------------
int mgdp_envs_set_explore(mgdp_envs *E, uint64_t seed0, const uint8_t *mask) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    return seed_streams(E, E->explore, seed0, mask, "mgdp_envs_set_explore");
}

int mgdp_envs_get_explore_streams(mgdp_envs *E, uint64_t *state, uint32_t *half) {
    MGDP_CHECK(E, MGDP_E_INVALID, "null handle");
    MGDP_CHECK(E->explore.on, MGDP_E_INVALID, "no explore streams on this handle (mgdp_envs_set_explore)");
    return read_streams(E, E->explore, state, half);
}

int mgdp_envs_q_learn_device(mgdp_envs *E, int32_t model, double *d_Q, int32_t n_steps, double alpha, double gamma,
                             double eps, int32_t n_act, int32_t unit_goal, int32_t *d_steps, int32_t *d_episodes,
                             int32_t *d_wins, double *d_ret, int32_t *d_status, int32_t *d_trace_state,
                             int8_t *d_trace_action, int32_t trace_len) {
    int S = 0, A = 0;
    if (int rc = q_learn_check(E, model, n_steps, alpha, gamma, eps, n_act, unit_goal, trace_len, &S, &A)) return rc;
    MGDP_CHECK(d_Q && d_steps && d_episodes && d_wins && d_ret && d_status, MGDP_E_INVALID, "null argument");
    TraceBufs t;
    if (int rc = trace_device(d_trace_state, d_trace_action, trace_len, &t)) return rc;
    DeviceGuard guard(E->device);
    const QLearnArgs q{d_Q, S, n_steps, n_act, unit_goal, t.len, alpha, gamma, eps, d_steps, d_episodes,
                       d_wins, d_ret, d_status, t.state, t.act};
    return launch_qlearn(E, model, q);
}

int mgdp_envs_q_learn(mgdp_envs *E, int32_t model, double *Q, int32_t n_steps, double alpha, double gamma, double eps,
                      int32_t n_act, int32_t unit_goal, int32_t *steps, int32_t *episodes, int32_t *wins, double *ret,
                      int32_t *status, int32_t *trace_state, int8_t *trace_action, int32_t trace_len) {
    int S = 0, A = 0;
    if (int rc = q_learn_check(E, model, n_steps, alpha, gamma, eps, n_act, unit_goal, trace_len, &S, &A)) return rc;
    MGDP_CHECK(Q, MGDP_E_INVALID, "null argument");
    TraceBufs h;  // the caller's buffers; none: no trace is taken
    if (int rc = trace_host(trace_state, trace_action, trace_len, &h)) return rc;
    DeviceGuard guard(E->device);
    const QLearnArgs q{nullptr, S, n_steps, n_act, unit_goal, 0, alpha, gamma, eps, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr};
    return q_learn_host(E, model, q, A, Q, steps, episodes, wins, ret, status, h);
}

int mgdp_envs_q_greedy_device(mgdp_envs *E, int32_t model, const double *d_Q, int32_t n_act, int8_t *d_pi, double *d_Vq) {
    int S = 0, A = 0;
    if (int rc = q_model_check(E, model, n_act, &S, &A)) return rc;
    MGDP_CHECK(d_Q && d_pi, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return launch_q_greedy(E, model, S, d_Q, n_act, d_pi, d_Vq);
}

int mgdp_envs_q_greedy(mgdp_envs *E, int32_t model, const double *Q, int32_t n_act, int8_t *pi, double *Vq) {
    int S = 0, A = 0;
    if (int rc = q_model_check(E, model, n_act, &S, &A)) return rc;
    MGDP_CHECK(Q && pi, MGDP_E_INVALID, "null argument");
    DeviceGuard guard(E->device);
    return q_greedy_host(E, model, S, A, Q, n_act, pi, Vq);
}

}  // extern "C"

