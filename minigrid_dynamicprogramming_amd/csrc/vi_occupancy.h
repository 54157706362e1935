// vi_occupancy.h -- the forward pass of a policy: the state distribution
// mu_{t+1} = P_pi^T mu_t of a stationary or time-indexed policy over exactly N steps, with the absorbed
// mass, the discounted visitation and the discounted reward collected on the way.  The transpose of
// vi_eval_fh_kernel's sweep on the same handle options (slip, NoDeath lava, finite horizon): XYD only,
// W*H <= 1024, one thread per cell.  Part of the single translation unit vi.hip (included after
// vi_eval_opts.h, whose policy-row ring and error word it reuses).
// Every product and sum below is one rounded operation in T in the order section 21 writes it (the
// library is built without FMA contraction); tests/occupancy_ref.py restates them on the oracle's tables.
#pragma once

namespace mgdp {

// The forward topology of one XYD cell, beside xyd_topo_soa's backward one: who sends into this cell.
// A neighbour outside the array is a wall: nothing here relies on the loader's rule that rim cells are not
// walkable, and a goal or lava cell on the rim looks behind itself out of the array.
template <typename T>
struct XydFwdTopo {
    int live;          // the agent may stand here: mass flows out of this cell
    int src[4];        // slot of the cell behind in dir d in a direction-major tile (own slot: none in the array)
    uint32_t in;       // bit d: the cell behind is live and its forward move from dir d lands here
    uint32_t blocked;  // bit d: this cell's own forward move from dir d stays where it is
    int pay;           // what entering pays: 0 nothing, 1 the goal reward, 2 the NoDeath lava cost
};

template <bool ND>
__device__ __forceinline__ bool xyd_stands(int t) { return xyd_free(t) || (ND && t == T_LAVA); }

template <typename T, bool ND>
__device__ __forceinline__ XydFwdTopo<T> xyd_fwd_topo_soa(const uint8_t *cl, const Geo &geo, int c) {
    XydFwdTopo<T> tp;
    const int x = c % geo.W, y = c / geo.W;
    const int t0 = cl[c];
    const bool enter = xyd_free(t0) || t0 == T_GOAL || t0 == T_LAVA;  // a forward move may land here
    tp.live = xyd_stands<ND>(t0);
    tp.pay = t0 == T_GOAL ? 1 : ((ND && t0 == T_LAVA) ? 2 : 0);
    tp.in = 0;
    tp.blocked = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int dx = d == 0 ? 1 : (d == 2 ? -1 : 0), dy = d == 1 ? 1 : (d == 3 ? -1 : 0);
        const int bx = x - dx, by = y - dy, fx = x + dx, fy = y + dy;
        const bool b_in = bx >= 0 && by >= 0 && bx < geo.W && by < geo.H;
        const bool f_in = fx >= 0 && fy >= 0 && fx < geo.W && fy < geo.H;
        const int bc = b_in ? by * geo.W + bx : c;
        const int tb = cl[bc];
        const int tf = cl[f_in ? fy * geo.W + fx : c];
        tp.src[d] = d * geo.HWs + bc;
        tp.in |= (uint32_t)(b_in && xyd_stands<ND>(tb) && enter) << d;
        tp.blocked |= (uint32_t)(tp.live && !(f_in && (xyd_free(tf) || tf == T_GOAL || tf == T_LAVA))) << d;
    }
    return tp;
}

// The start error word, folded with atomicMin: {grid : 32 | state : 32} -- the lowest grid, its lowest state.
__device__ __forceinline__ void start_report(unsigned long long *serr, int e, unsigned int s) {
    atomicMin(serr, ((unsigned long long)e << 32) | (unsigned long long)s);
}

// ------------------------------------------------------------------------------------------------
// One workgroup per grid, one thread per cell -- goal, lava and wall cells too (idle threads shadow cell 0
// and never write HBM).  A thread keeps its cell's four masses, its occ and its ret accumulators in
// registers.  Step t: every thread writes its four forward outflows f(., 2) to its slot of a
// direction-major tile, and after the step's one barrier reads the outflow of the cell behind it in each
// direction -- xyd_load_nb's exchange transposed, tiles double-buffered (a tile is written again two
// barriers after it was read).  Exactly N steps, no stop test.
// tab: T [3][N] = disc, wg (the discounted goal reward), wl (the discounted NoDeath lava cost).
// TI: pi_src is [N][B][S], t-major, read ascending through vi_eval_fh_kernel's register ring; a row's
// lanes are checked as they are consumed, and an offending cell raises the step's stop word (one of two, by
// step parity), which every thread reads behind the step's barrier: the grid then steps no further.  The
// error word is section 19's with the row field holding t itself, so atomicMin keeps the smallest offending t.
// !TI: pi_src is [B][S], checked once.
// MT: every mu_t into mu_t as T [N][B][S]; a thread stores its own cell's slice from registers.
// ------------------------------------------------------------------------------------------------
template <typename T, bool SLIP, bool ND, bool TI, bool MT>
__global__ void __launch_bounds__(1024)
vi_occupancy_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, const int8_t *pi_src,
                    const int32_t *__restrict__ start, const T *__restrict__ mu0, const T *__restrict__ tab,
                    T *__restrict__ mu_out, T *__restrict__ occ_out, T *__restrict__ ret_out, T *__restrict__ mu_t,
                    unsigned long long *__restrict__ everr, int N) {
    constexpr int PF = kEvalPrefetch;
    constexpr int M = MGDP_MODEL_XYD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem L = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), 2);
    T *F0 = reinterpret_cast<T *>(smem);
    T *F1 = reinterpret_cast<T *>(smem + L.v_bytes);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + L.cells_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + L.flags_off());
    uint32_t *stopw = reinterpret_cast<uint32_t *>(flags + 32);  // step t raises stopw[t & 1], and reads it behind its barrier
    const int e = blockIdx.x, tid = threadIdx.x, HWs = geo.HWs;
    const bool own_cell = tid < geo.HW;
    const int cc = own_cell ? tid : 0;
    const long long vb = (long long)e * geo.S, BS = (long long)geo.B * geo.S;
    copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
    if (tid < 64) flags[tid] = 0;
    __syncthreads();
    const XydFwdTopo<T> tp = xyd_fwd_topo_soa<T, ND>(cl, geo, cc);
    const uint32_t vmask = tp.live ? 0x80808080u : 0u;
    const int8_t *prow = pi_src + vb + (long long)cc * 4;
    const T *disc = tab, *wgt = tab + N, *wlt = tab + 2 * (long long)N;

    // mu_0: a one-hot start state or the caller's distribution; walls, goal and terminal lava hold no mass
    T mu[4], occ[4], ret[4];
    if (mu0) {
        const V4<T> m = *reinterpret_cast<const V4<T> *>(mu0 + vb + (long long)cc * 4);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (!tp.live && m.v[d] != (T)0) start_report(everr + 1, e, (unsigned int)(cc * 4 + d));
            mu[d] = tp.live ? m.v[d] : (T)0;
        }
    } else {
        const int s0 = start[e];
        const bool ok = s0 >= 0 && s0 < geo.S && xyd_stands<ND>(cl[(s0 >= 0 && s0 < geo.S) ? (s0 >> 2) : 0]);
        if (!ok && tid == 0) start_report(everr + 1, e, (unsigned int)s0);
#pragma unroll
        for (int d = 0; d < 4; ++d) mu[d] = (ok && s0 == cc * 4 + d) ? (T)1 : (T)0;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) occ[d] = ret[d] = (T)0;

    PkN<M> pk0 = {}, ring[PF];
    // (two rings of workgroup-uniform weights, selected per cell at use: one ring read through a per-cell pointer
    // turns the scalar loads into vector loads, and the fp64 slip kernels with mu_t then spill 40-72 B a lane)
    T dsc[PF], wgs[PF], wls[PF];  // the rows' discount and reward weights ride the same ring (vi_eval_fh_kernel's rgs)
    bool stop = false;
#pragma unroll
    for (int j = 0; j < PF; ++j) {  // (unconditional loads in ring order, a row past the end clamped to the last)
        const int tr = j < N ? j : N - 1;
        dsc[j] = disc[tr];
        wgs[j] = wgt[tr];
        wls[j] = ND ? wlt[tr] : (T)0;
        if constexpr (TI) ring[j] = load_pk<M>(prow + (long long)tr * BS);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!TI) {
        pk0 = load_pk<M>(prow);
        const bool bad = lanes_bad<M>(pk0, vmask);
        if (bad) lanes_report<M>(pk0, vmask, e, 0, cc, everr);
        stop = __builtin_amdgcn_readfirstlane((int)block_any(bad, flags, 1)) != 0;
    }
    int tbad = -1;  // TI: the step whose row offended in this cell
    const T w = cf.p + cf.c;  // slip: the weight of the chosen action among a' <= 5
    T *Fout = F0, *Fnext = F1;
    int Nrun = stop ? 0 : N;
    // One step on ring slot j; the loop's shape (full rounds of PF steps that refill their slots, the last
    // N mod PF steps from the ring, a raised stop word ending the loop through Nrun) is vi_eval_fh_kernel's.
    auto step = [&](int j, int t, bool refill) __attribute__((always_inline)) {
        uint32_t pk = TI ? ring[j].w[0] : pk0.w[0];
        // (the stationary slip lanes made opaque per step, as vi_eval_fh_kernel does for DoorKey: the compiler
        // otherwise hoists the slip form's 28 lane compares out of the loop into more SGPR pairs than it has,
        // and spills them through v_writelane / v_readlane inside every step -- 22 to 62 SGPR spills.  The
        // deterministic form's compares fit, and stay hoisted.)
        if constexpr (!TI && SLIP) asm volatile("" : "+v"(pk));
        const T dt = dsc[j], wg = wgs[j], wl = wls[j];
        const bool dead = TI && Nrun == 0;
        if constexpr (TI) {
            // (reported behind the loop: an atomic in it joins the row loads on the vector-memory counter)
            if (lanes_bad<M>(ring[j], vmask) && !dead) {
                tbad = t;
                stopw[t & 1] = 1u;
            }
        }
        if constexpr (MT) {  // row t: mu_t on live states, the mass absorbed so far on terminal ones
            if (own_cell && !dead)
                *reinterpret_cast<V4<T> *>(mu_t + (long long)t * BS + vb + (long long)tid * 4) = V4<T>{{mu[0], mu[1], mu[2], mu[3]}};
        }
        // Slip: an outflow is one product, coefficient selected first -- fl(w*m) for the chosen action, fl(c*m)
        // for any other a' <= 5 -- so only the live masses cross the barrier, and a share that several sums take
        // is multiplied again rather than kept (fp64: the kept shares were 24 more VGPRs, and spilled).
        auto share = [&](uint32_t ad, uint32_t k, T m) __attribute__((always_inline)) {
            if (SLIP) return (ad == k ? w : cf.c) * m;
            return ad == k ? m : (T)0;
        };
        uint32_t a[4];
        T lm[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            a[d] = (pk >> (8 * d)) & 0xffu;
            lm[d] = tp.live ? mu[d] : (T)0;
            Fout[d * HWs + tid] = share(a[d], 2u, lm[d]);  // f(s, 2)
            occ[d] = occ[d] + dt * lm[d];
        }
        // the ring slot is refilled after the row's last use
        if (refill) {
            const int tr = t + PF < N ? t + PF : N - 1;
            dsc[j] = disc[tr];
            wgs[j] = wgt[tr];
            wls[j] = ND ? wlt[tr] : (T)0;
            if constexpr (TI) ring[j] = load_pk<M>(prow + (long long)tr * BS);
        }
        __syncthreads();
        uint32_t st = 0;
        if constexpr (TI) st = stopw[t & 1];
        T fin[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) fin[d] = Fout[tp.src[d]];
        if (TI && __builtin_amdgcn_readfirstlane((int)st) != 0) Nrun = 0;
        const T om = tp.pay == 1 ? wg : wl;
        T nm[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int dl = (d + 1) & 3, dr = (d + 3) & 3;  // left from d+1 and right from d-1 turn into d
            const T Fin = ((tp.in >> d) & 1u) ? fin[d] : (T)0;
            T s = share(a[dl], 0u, lm[dl]) + share(a[dr], 1u, lm[dr]);
            s = s + Fin;
            if (SLIP) {
                s = s + (((tp.blocked >> d) & 1u) ? share(a[d], 2u, lm[d]) : (T)0);
                s = s + share(a[d], 3u, lm[d]);
                s = s + share(a[d], 4u, lm[d]);
                s = s + share(a[d], 5u, lm[d]);
                const T pm = cf.p * lm[d];
                s = s + (a[d] == 6u ? pm : (T)0);
            } else {
                // (at most one of Fself, f(s',3) .. f(s',6) is not +0, and x + +0 = x: one addition gives the
                // sum of the five taken left to right)
                const bool self = a[d] == 2u ? ((tp.blocked >> d) & 1u) != 0u : (a[d] >= 3u && a[d] <= 6u);
                s = s + (self ? lm[d] : (T)0);
            }
            nm[d] = tp.live ? s : mu[d] + Fin;  // terminal states keep what they absorbed; walls receive +0
            ret[d] = tp.pay ? ret[d] + om * Fin : (T)0;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) mu[d] = nm[d];
        T *x = Fout;
        Fout = Fnext;
        Fnext = x;
    };
    int t0 = 0;
    for (; t0 + PF <= Nrun; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) step(j, t0 + j, true);
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        if (t0 + j >= Nrun) break;
        step(j, t0 + j, false);
    }
    if constexpr (TI) {
        // (the offending row is read once more rather than carried through the loop)
        if (tbad >= 0) lanes_report<M>(load_pk<M>(prow + (long long)tbad * BS), vmask, e, tbad, cc, everr);
    }
    if (own_cell) {
        const long long o = vb + (long long)tid * 4;
        *reinterpret_cast<V4<T> *>(mu_out + o) = V4<T>{{mu[0], mu[1], mu[2], mu[3]}};
        if (occ_out) *reinterpret_cast<V4<T> *>(occ_out + o) = V4<T>{{occ[0], occ[1], occ[2], occ[3]}};
        if (ret_out) *reinterpret_cast<V4<T> *>(ret_out + o) = V4<T>{{ret[0], ret[1], ret[2], ret[3]}};
    }
}

}  // namespace mgdp
