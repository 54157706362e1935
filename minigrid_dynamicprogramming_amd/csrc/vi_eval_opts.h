// vi_eval_opts.h -- policy evaluation under the handle options: V^pi on NoDeath
// lava (discounted, the protocol of vi_eval_kernel), the finite-horizon backward induction of a
// stationary or time-indexed policy (exactly H sweeps, no stop test).  (The greedy improvement on the
// NoDeath Q is vi_improve_kernel's ND form, vi_eval.h.)  Part of the single translation unit vi.hip
// (included after vi_eval.h).  Option handles hold W*H <= 1024 (mgdp_vi_create), so every kernel here is one thread per cell, topology
// and lanes in registers, both V tiles in LDS (smem_layout's direction-major tiles).
// The steps are the per-action forms Qd = done ? R : fl(R + fl(g*V[s'])) of the oracle's tables: V may
// be negative under NoDeath, so none of xyd_step's value-only shortcuts (max with +0, an invalid front
// reading +0) is used.
#pragma once

namespace mgdp {

// Rows of a time-indexed policy loaded ahead of the sweep that consumes them (compile time: the ring
// lives in registers).  Measured at 1 / 2 / 4 / 8: 2 was the best or tied on every
// workload; 1 exposes the load, 4 and 8 gain nothing and cost registers and code.
#ifndef MGDP_EVAL_PF
#define MGDP_EVAL_PF 2
#endif
constexpr int kEvalPrefetch = MGDP_EVAL_PF;

// The finite-horizon policy error word, folded with atomicMin: {grid : 22 | H-1-t : 20 | state : 14 |
// action : 8} -- the lowest offending grid, its largest offending t, that row's lowest offending state.
constexpr int kFhRowShift = 22, kFhGridShift = 42;
constexpr int kFhMaxH = 1 << 20, kFhMaxB = (1 << 22) - 1;

template <int MODEL> struct PkN { uint32_t w[MODEL == MGDP_MODEL_XYD ? 1 : 4]; };
template <typename T, int MODEL> struct CellV { T v[MODEL == MGDP_MODEL_XYD ? 4 : 16]; };

template <int MODEL>
__device__ __forceinline__ PkN<MODEL> load_pk(const int8_t *p) {
    PkN<MODEL> pk;
    if constexpr (MODEL == MGDP_MODEL_XYD) {
        pk.w[0] = *reinterpret_cast<const uint32_t *>(p);
    } else {
        const uint4 r = *reinterpret_cast<const uint4 *>(p);
        pk.w[0] = r.x, pk.w[1] = r.y, pk.w[2] = r.z, pk.w[3] = r.w;
    }
    return pk;
}
template <int MODEL>
__device__ __forceinline__ void store_pk(int8_t *p, const PkN<MODEL> &pk) {
    if constexpr (MODEL == MGDP_MODEL_XYD) *reinterpret_cast<uint32_t *>(p) = pk.w[0];
    else *reinterpret_cast<uint4 *>(p) = make_uint4(pk.w[0], pk.w[1], pk.w[2], pk.w[3]);
}

// bit 7 of every byte of pk that is >= A as an unsigned value (A <= 128; no carry between bytes)
__device__ __forceinline__ uint32_t lanes_ge(uint32_t pk, uint32_t A) {
    return (((pk & 0x7f7f7f7fu) + (0x80u - A) * 0x01010101u) | pk) & 0x80808080u;
}
// bit 7 of every byte whose lane belongs to a valid state.  XYD: the cell's four directions at once;
// DoorKey: byte hd = has_key*2 + door_open of each direction's word.
template <typename T>
__device__ __forceinline__ uint32_t lane_mask(const XydTopo<T> &tp) { return tp.valid ? 0x80808080u : 0u; }
__device__ __forceinline__ uint32_t lane_mask(const DkTopo &tp) {
    uint32_t m = 0;
#pragma unroll
    for (int hd = 0; hd < 4; ++hd) m |= ((tp.walk >> hd) & 1u) << (8 * hd + 7);
    return m;
}
template <int MODEL>
__device__ __forceinline__ bool lanes_bad(const PkN<MODEL> &pk, uint32_t vmask) {
    constexpr uint32_t A = MODEL == MGDP_MODEL_XYD ? 7u : 5u;
    uint32_t b = 0;
#pragma unroll
    for (int q = 0; q < (MODEL == MGDP_MODEL_XYD ? 1 : 4); ++q) b |= lanes_ge(pk.w[q], A) & vmask;
    return b != 0u;
}
// the lanes as stored: absorbing states -1
template <int MODEL>
__device__ __forceinline__ PkN<MODEL> lanes_norm(PkN<MODEL> pk, uint32_t vmask) {
    const uint32_t inv = ((~vmask & 0x80808080u) >> 7) * 0xffu;
#pragma unroll
    for (int q = 0; q < (MODEL == MGDP_MODEL_XYD ? 1 : 4); ++q) pk.w[q] |= inv;
    return pk;
}
// the rare path: every offending lane of the cell into the error word
template <int MODEL>
__device__ __forceinline__ void lanes_report(const PkN<MODEL> &pk, uint32_t vmask, int e, int row, int c,
                                             unsigned long long *everr) {
    constexpr int NL = MODEL == MGDP_MODEL_XYD ? 4 : 16;
    constexpr uint32_t A = MODEL == MGDP_MODEL_XYD ? 7u : 5u;
    for (int l = 0; l < NL; ++l) {
        const uint32_t a = (pk.w[l >> 2] >> (8 * (l & 3))) & 0xffu;
        if (((vmask >> (8 * (l & 3) + 7)) & 1u) && a >= A)
            atomicMin(everr, ((unsigned long long)e << kFhGridShift) | ((unsigned long long)row << kFhRowShift) |
                                 ((unsigned long long)(c * NL + l) << 8) | a);
    }
}

// ------------------------------------------------------------------------------------------------
// The evaluation step of one XYD cell under the options: xyd_eval_step with the NoDeath lava move
// (ND: fl(dc + fl(g*x)) for a forward move into lava -- the operand is still selected first and
// multiplied once) and the finite-horizon goal reward (FH: rg in place of 1).  Slip: xyd_slip_tail's chain.
// ------------------------------------------------------------------------------------------------
template <typename T, bool SLIP, bool ND, bool FH>
__device__ __forceinline__ void xyd_eval_step_opts(const XydTopo<T> &tp, const Coef<T> &cf, const T (&own)[4],
                                                   const T (&nbv)[4], uint32_t pk, T rg, T (&out)[4]) {
    if (!SLIP) {
        // (the own values as scalars: a select chain over the array's elements became one indexed load
        // from a private copy of the array, 16 B of scratch)
        const T o0 = own[0], o1 = own[1], o2 = own[2], o3 = own[3];
        const T oL[4] = {o3, o0, o1, o2}, oR[4] = {o1, o2, o3, o0}, oS[4] = {o0, o1, o2, o3};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t a = (pk >> (8 * d)) & 0xffu;
            // (one flat select per action, not a nested chain: the chain became divergent branches)
            T x = oS[d];
            x = a == 2u ? nbv[d] : x;
            x = a == 1u ? oR[d] : x;
            x = a == 0u ? oL[d] : x;
            T q = cf.g * x;
            if (ND) q = (a == 2u && ((tp.lavaF >> d) & 1u)) ? cf.dc + q : q;
            q = (a == 2u && ((tp.term >> d) & 1u)) ? (FH ? tp.tq[d] * rg : tp.tq[d]) : q;
            out[d] = tp.valid ? q : (T)0;
        }
        return;
    }
    T gv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) gv[d] = cf.g * own[d];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t a = (pk >> (8 * d)) & 0xffu;
        // (xyd_forward<T, ND, FH> restated: through it the slip NoDeath kernels changed their register assignment)
        const T qM = (ND && ((tp.lavaF >> d) & 1u)) ? cf.dc + cf.g * nbv[d] : cf.g * nbv[d];
        const T qF = ((tp.term >> d) & 1u) ? (FH ? tp.tq[d] * rg : tp.tq[d]) : qM;
        const T qL = gv[(d + 3) & 3], qR = gv[(d + 1) & 3], qS = gv[d];
        const T tail = xyd_slip_tail(cf, qL, qR, qF, qS);
        T qa = qS;
        qa = a == 2u ? qF : qa;
        qa = a == 1u ? qR : qa;
        qa = a == 0u ? qL : qa;
        const T best = cf.p * qa + tail;
        out[d] = tp.valid ? best : (T)0;  // slip mixes in constants; absorbing states stay 0
    }
}

// dk_eval_step with the finite-horizon goal reward
template <typename T>
__device__ __forceinline__ void dk_eval_step_fh(const DkTopo &tp, const Coef<T> &cf, const T (&own)[16],
                                                const V4<T> (&nbs)[4], const uint32_t (&pk)[4], T rg, T (&outv)[16]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t f = tp.f[d];
        const V4<T> &nb = nbs[d];
        const bool goal = f & 16u, lava = f & 32u;
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) {
#pragma unroll
            for (int dop = 0; dop < 2; ++dop) {
                const int l = (d * 2 + hk) * 2 + dop;
                const int hd = hk * 2 + dop;
                const uint32_t a = (pk[l >> 2] >> (8 * (l & 3))) & 0xffu;
                const T xS = own[l];
                const T xL = own[((d + 3) & 3) * 4 + hd];
                const T xR = own[((d + 1) & 3) * 4 + hd];
                T xM, xP, xT;
                dk_reads(f, hk, dop, own + d * 4, nb.v[hd], xM, xP, xT);
                T x = xS;
                x = a == 4u ? xT : x;
                x = a == 3u ? xP : x;
                x = a == 2u ? xM : x;
                x = a == 1u ? xR : x;
                x = a == 0u ? xL : x;
                T q = cf.g * x;
                const T qt = goal ? rg : (T)0;  // a terminal front: dk_forward<T, true> (vi_model.h) as one flat select
                q = (a == 2u && (goal || lava)) ? qt : q;
                outv[l] = ((tp.walk >> hd) & 1u) ? q : (T)0;
            }
        }
    }
}

// a cell's values: register set <-> its slot of a direction-major LDS tile / its slice of an HBM row
template <typename T, int MODEL>
__device__ __forceinline__ void cell_to_tile(T *tile, const CellV<T, MODEL> &x, int HWs, int c) {
    if constexpr (MODEL == MGDP_MODEL_XYD) {
#pragma unroll
        for (int d = 0; d < 4; ++d) tile[d * HWs + c] = x.v[d];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<V4<T> *>(tile + (q * HWs + c) * 4) = V4<T>{{x.v[4 * q], x.v[4 * q + 1], x.v[4 * q + 2], x.v[4 * q + 3]}};
    }
}
template <typename T, int MODEL>
__device__ __forceinline__ void cell_to_row(T *row, const CellV<T, MODEL> &x, int c) {
    constexpr int NQ = MODEL == MGDP_MODEL_XYD ? 1 : 4;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        *reinterpret_cast<V4<T> *>(row + c * (4 * NQ) + 4 * q) = V4<T>{{x.v[4 * q], x.v[4 * q + 1], x.v[4 * q + 2], x.v[4 * q + 3]}};
}

template <typename T, bool SLIP, bool ND>
__device__ __forceinline__ void fh_cell(const XydTopo<T> &tp, const Coef<T> &cf, const CellV<T, MGDP_MODEL_XYD> &own,
                                        const T *Vin, const PkN<MGDP_MODEL_XYD> &pk, T rg, CellV<T, MGDP_MODEL_XYD> &out) {
    T nbv[4];
    xyd_load_nb(tp, Vin, nbv);
    // (the front values pinned in registers: left to itself the compiler turned the step's select chains
    // into divergent branches with the LDS reads sunk into them)
    asm volatile("" : "+v"(nbv[0]), "+v"(nbv[1]), "+v"(nbv[2]), "+v"(nbv[3]));
    xyd_eval_step_opts<T, SLIP, ND, true>(tp, cf, own.v, nbv, pk.w[0], rg, out.v);
}
template <typename T, bool SLIP, bool ND>
__device__ __forceinline__ void fh_cell(const DkTopo &tp, const Coef<T> &cf, const CellV<T, MGDP_MODEL_DOORKEY> &own,
                                        const T *Vin, const PkN<MGDP_MODEL_DOORKEY> &pk, T rg,
                                        CellV<T, MGDP_MODEL_DOORKEY> &out) {
    V4<T> nbs[4];
    dk_load_nb(tp, Vin, nbs);
#pragma unroll
    for (int d = 0; d < 4; ++d) asm volatile("" : "+v"(nbs[d].v[0]), "+v"(nbs[d].v[1]), "+v"(nbs[d].v[2]), "+v"(nbs[d].v[3]));
    dk_eval_step_fh<T>(tp, cf, own.v, nbs, pk.w, rg, out.v);
}

// ------------------------------------------------------------------------------------------------
// Finite-horizon evaluation, one workgroup per grid, one thread per cell (idle threads shadow cell 0
// and never write HBM): V_H = 0, then sweep k = 0 .. H-1 computes V_t, t = H-1-k, from V_{t+1} with the
// goal reward rgoal[t] and the lanes pi_t -- one barrier per sweep, no stop test.  A thread keeps its
// cell's V_{t+1} in registers (the tiles serve the neighbours only); |dV| is taken at the last sweep only.
// TI: pi_src is [H][B][S], t-major; a cell's lanes of row t are its thread's own 4 / 16 bytes, loaded
// kEvalPrefetch sweeps ahead into a register ring (the only per-sweep HBM read; it waits under the
// barrier chain).  A row's lanes are checked as they are consumed: an offending cell reports into
// *everr and raises the sweep's stop word (one of two, by sweep parity), which every thread reads after the
// sweep's barrier, with the next sweep's neighbour values -- the grid then sweeps nothing further (that next
// sweep stores and counts nothing and ends the loop, in every wave alike).
// !TI: pi_src is [B][S], checked and normalised once, kept in registers for all H sweeps.
// VT: every V_t into Vt as T [H][B][S]; a thread stores its own cell's slice from registers.  (With TI the
// stores share the loads' counter, and the compiler waits for both at each row's first use.)
// pi receives the normalised pi_0; V the final V_0; kenv / kexec H; dvenv max|V_0 - V_1|.
// ------------------------------------------------------------------------------------------------
// The workgroup bound: 1024 threads, but an fp64 DoorKey grid whose two V tiles fit a CU's LDS (160 KiB:
// 2 * 16 * 8 B + 16 B a cell) has at most 576 cell slots -- 640 leaves its 16-state fp64 step 168 VGPRs.
template <typename T, int MODEL>
constexpr int kEvalFhBlock = (MODEL == MGDP_MODEL_DOORKEY && sizeof(T) == 8) ? 640 : 1024;

template <typename T, int MODEL, bool SLIP, bool ND, bool TI, bool VT>
__global__ void __launch_bounds__((kEvalFhBlock<T, MODEL>))
vi_eval_fh_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V, const int8_t *pi_src,
                  int8_t *pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                  unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
                  unsigned long long *__restrict__ host_out, unsigned long long *__restrict__ everr,
                  const T *__restrict__ rgoal, T *__restrict__ Vt, int H, int in_kernel_reduce, unsigned int epoch) {
    constexpr int NS = MODEL == MGDP_MODEL_XYD ? 4 : 16;
    constexpr int PF = kEvalPrefetch;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem L = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), 2);
    T *V0 = reinterpret_cast<T *>(smem);
    T *V1 = reinterpret_cast<T *>(smem + L.v_bytes);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + L.cells_off());
    T *slots = reinterpret_cast<T *>(smem + L.slots_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + L.flags_off());
    // two stop words behind block_any's two parities, alternated by sweep parity as flag_write's flags are:
    // sweep k raises stopw[k & 1] and reads stopw[(k - 1) & 1], so a sweep observes the previous sweep's word only
    uint32_t *stopw = reinterpret_cast<uint32_t *>(flags + 32);
    const int e = blockIdx.x, tid = threadIdx.x, HWs = geo.HWs;
    const bool own_cell = tid < geo.HW;
    const int cc = own_cell ? tid : 0;
    const long long vb = (long long)e * geo.S, BS = (long long)geo.B * geo.S;
    copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
    if (tid < 64) flags[tid] = 0;
    zero16(V0, 2 * L.v_bytes);
    __syncthreads();
    typename TopoOf<T, MODEL>::type tp;
    if constexpr (MODEL == MGDP_MODEL_XYD) tp = xyd_topo_soa<T, ND>(cl, geo, cc);
    else tp = dk_topo_soa(cl, geo, cc);
    const uint32_t vmask = lane_mask(tp);
    const int8_t *prow = pi_src + vb + (long long)cc * NS;
    PkN<MODEL> pk0 = {}, ring[PF];
    T rgs[PF];  // the rows' goal rewards ride the same ring, as vector loads: they return in order, off the LDS counter
    bool stop = false;
#pragma unroll
    for (int j = 0; j < PF; ++j) {  // (every ring load is unconditional, a row index below 0 clamped to row 0:
        const int tr = H - 1 - j > 0 ? H - 1 - j : 0;  // behind a branch the compiler cannot count the loads in
        rgs[j] = rgoal[tr];                            // flight, and waits for all of them at every use)
        if constexpr (TI) ring[j] = load_pk<MODEL>(prow + (long long)tr * BS);
        // (issued in ring order: the loop's first wait is for slot 0, and with slot 0 loaded last here --
        // the scheduler's choice -- it became a wait for every load, at the loop head of every round)
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!TI) {
        pk0 = load_pk<MODEL>(prow);
        const bool bad = lanes_bad<MODEL>(pk0, vmask);
        if (bad) lanes_report<MODEL>(pk0, vmask, e, 0, cc, everr);
        pk0 = lanes_norm<MODEL>(pk0, vmask);
        if (own_cell) store_pk<MODEL>(pi + vb + (long long)tid * NS, pk0);
        stop = __builtin_amdgcn_readfirstlane((int)block_any(bad, flags, 1)) != 0;
    }
    int kbad = -1;  // TI: the sweep whose row offended in this cell
    CellV<T, MODEL> own, out;
#pragma unroll
    for (int i = 0; i < NS; ++i) own.v[i] = (T)0;
    T *Vin = V0, *Vout = V1;
    T diff = (T)0;
    // (the loop's state is kept wave-uniform for the compiler, so its branches stay scalar)
    int k = 0;
    // One sweep on ring slot j (k = sweep index).  Full rounds of PF sweeps run with no exit inside the
    // round and refill their slots; the last H mod PF sweeps find their rows in the ring already.  (With an
    // exit inside the round, or a refill behind a branch, the compiler cannot count the row loads in flight
    // and waits for all of them at each row's first use.)  A raised stop word ends the loop through Hrun; a
    // sweep that sees it stores and counts nothing.  `dead` is the same in every wave: the word a sweep reads
    // was written before the previous sweep's barrier and is not written again before this sweep's (the other
    // word is), and once seen it stays in Hrun (the sweeps left in the round read the other, never raised word).
    int Hrun = stop ? 0 : H;
    auto sweep = [&](int j, int kk, bool refill) __attribute__((always_inline)) {
        const int t = H - 1 - kk;
        PkN<MODEL> pk = pk0;
        uint32_t st = 0;
        const T rg = rgs[j];
        if constexpr (TI) {
            pk = ring[j];
            st = stopw[(kk & 1) ^ 1];
        } else if constexpr (MODEL == MGDP_MODEL_DOORKEY) {
            // (the stationary lanes made opaque per sweep: the compiler otherwise hoists DoorKey's 80 lane
            // compares out of the loop into SGPR pairs it does not have, and spills them through
            // v_writelane / v_readlane inside every sweep -- 703 readlanes in the fp32 kernel, and slower
            // than the time-indexed form that decodes its row every sweep)
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(pk.w[q]));
        }
        fh_cell<T, SLIP, ND>(tp, cf, own, Vin, pk, rg, out);
        if (TI && __builtin_amdgcn_readfirstlane((int)st) != 0) Hrun = 0;
        const bool dead = TI && Hrun == 0;
        if constexpr (TI) {
            // (reported and stored behind the loop: a store or an atomic in it joins the row loads on the
            // vector-memory counter, and the compiler then waits for all of them every sweep)
            if (lanes_bad<MODEL>(pk, vmask) && !dead) {
                kbad = kk;
                stopw[kk & 1] = 1u;
            }
        }
        cell_to_tile<T, MODEL>(Vout, out, HWs, tid);
        if constexpr (VT) {
            if (own_cell && !dead) cell_to_row<T, MODEL>(Vt + (long long)t * BS + vb, out, tid);
        }
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) diff = vmax(diff, vabs(out.v[i] - own.v[i]));
        }
        // the ring slot is refilled after the row's last use: its registers then never hold two rows at once
        if (refill) {
            const int tr = t >= PF ? t - PF : 0;
            rgs[j] = rgoal[tr];
            if constexpr (TI) ring[j] = load_pk<MODEL>(prow + (long long)tr * BS);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NS; ++i) own.v[i] = out.v[i];
        T *x = Vin;
        Vin = Vout;
        Vout = x;
        k += dead ? 0 : 1;
    };
    int k0 = 0;
    for (; k0 + PF <= Hrun; k0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) sweep(j, k0 + j, true);
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        if (k0 + j >= Hrun) break;
        sweep(j, k0 + j, false);
    }
    if constexpr (TI) {
        // (the offending row and row 0 are read once more rather than carried through the loop)
        if (kbad >= 0) lanes_report<MODEL>(load_pk<MODEL>(prow + (long long)(H - 1 - kbad) * BS), vmask, e, kbad, cc, everr);
        if (k == H && own_cell) store_pk<MODEL>(pi + vb + (long long)tid * NS, lanes_norm<MODEL>(load_pk<MODEL>(prow), vmask));
    }
    const double dvl = (double)block_max(diff, slots, 0);
    if (own_cell) cell_to_row<T, MODEL>(V + vb, own, tid);
    record_grid(geo, kenv, dvenv, e, k, dvl, tid == 0);
    if (in_kernel_reduce)
        fused_reduce(red, ticket, host_out, k, dvl, reinterpret_cast<unsigned int *>(slots + 16), epoch, false, tid);
}

// ------------------------------------------------------------------------------------------------
// Discounted V^pi on NoDeath lava: vi_eval_kernel's protocol (own rule / run-to, fresh, kenv / dvenv,
// fixed-point completion, the policy resolved and checked at the fresh launch) on the NoDeath
// topology and step.  XYD, W*H <= 1024: the register form only.
// ------------------------------------------------------------------------------------------------
template <typename T, bool SLIP>
__global__ void __launch_bounds__(1024)
vi_eval_nd_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V, const int8_t *pi_src,
                  int8_t *pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
                  unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
                  unsigned long long *__restrict__ host_out, unsigned long long *__restrict__ everr, int k_target,
                  int fresh, int in_kernel_reduce, unsigned int epoch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem L = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), 2);
    T *V0 = reinterpret_cast<T *>(smem);
    T *V1 = reinterpret_cast<T *>(smem + L.v_bytes);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + L.cells_off());
    T *slots = reinterpret_cast<T *>(smem + L.slots_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + L.flags_off());
    const int e = blockIdx.x, tid = threadIdx.x, HW = geo.HW, HWs = geo.HWs;
    int k = fresh ? 0 : kenv[e];
    double dvl = fresh ? 0.0 : dvenv[e];
    if (k_target > k && k > 0 && dvl == 0.0) {  // fixed-point completion (grid_complete_at)
        if (tid == 0) kenv[e] = k_target;
        k = k_target;
    }
    const bool own_rule = k_target < 0;
    const bool work = own_rule ? (!(k > 0 && dvl < geo.tol) && k < geo.max_sweeps) : (k < k_target);
    if (work) {
        const long long vb = (long long)e * geo.S;
        T *Vg = V + vb;
        copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
        if (tid < 64) flags[tid] = 0;
        if (k == 0) {
            zero16(V0, 2 * L.v_bytes);
        } else {
            if (tid < HW) eval_load_cell<T, MGDP_MODEL_XYD>(V0, Vg, HWs, tid);
        }
        __syncthreads();
        XydTopo<T> tp = {};
        uint32_t pk = 0;
        bool bad = false;
        if (tid < HW) {
            tp = xyd_topo_soa<T, true>(cl, geo, tid);
            if (fresh) pk = resolve_pi(tp, pi_src + vb, pi + vb, tid, e, everr, bad);
            else pk = *reinterpret_cast<const uint32_t *>(pi + vb + (long long)tid * 4);
        }
        if (block_any(bad, flags, 1)) {
            k = 0;
            dvl = 0.0;
        } else {
            T *Vin = V0, *Vout = V1;
            int parity = 0;
            T diff = (T)0;
            while (own_rule ? k < geo.max_sweeps : k < k_target) {
                T d = (T)0;
                if (tid < HW) {
                    T own[4], out[4], nbv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) own[q] = Vin[q * HWs + tid];
                    xyd_load_nb(tp, Vin, nbv);
                    xyd_eval_step_opts<T, SLIP, true, false>(tp, cf, own, nbv, pk, (T)1, out);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        Vout[q * HWs + tid] = out[q];
                        d = vmax(d, vabs(out[q] - own[q]));
                    }
                }
                diff = d;
                flag_write(d >= cf.tol, flags, parity);
                __syncthreads();
                ++k;
                T *t = Vin;
                Vin = Vout;
                Vout = t;
                const bool more = flags_any(flags, parity);
                parity ^= 1;
                if (own_rule && !more) break;
            }
            dvl = (double)block_max(diff, slots, 0);
            if (tid < HW) eval_store_cell<T, MGDP_MODEL_XYD>(Vg, Vin, HWs, tid);
        }
        record_grid(geo, kenv, dvenv, e, k, dvl, tid == 0);
    }
    if (in_kernel_reduce)
        fused_reduce(red, ticket, host_out, k, dvl, reinterpret_cast<unsigned int *>(slots + 16), epoch, false, tid);
}

}  // namespace mgdp
