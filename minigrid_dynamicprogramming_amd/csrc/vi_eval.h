// vi_eval.h -- policy evaluation and greedy improvement: V^pi of a given
// policy by Jacobi sweeps under the stopping rule of the solve, and pi' = argmax_a Q on the handle's V.
// Part of the single translation unit vi.hip (included after vi_kernels.h).  The steps take the
// per-action values from vi_model.h's one statement of them (xyd_forward, xyd_slip_tail / xyd_mix,
// dk_reads / dk_forward / dk_q5, q_argmax) with Q[pi(s)] in place of the max over actions, so every
// Q is bit-identical to the table form Qd = done ? R : fl(R + g*V[s']) of the oracle's tables.
#pragma once

namespace mgdp {

// The evaluation's launch shape, its own (plan_vi / ViPlan describe the solve only): one workgroup per
// grid, one thread per cell up to 1024 cells and the cells strided over 1024 threads above; LDS =
// smem_layout's [2 V tiles][packed pi][cells][slots, flags] on direction-major tiles of stride HWs
// (a slot per thread up to 1024 cells; above, only cells are addressed and the planes are not padded).
struct EvalShape {
    int block, HWs, Ss, lds;
    int improve_block, improve_lds;  // vi_improve_kernel: [V row, cell-major][cells]
};
inline EvalShape eval_shape(int HW, int HWp, int S, int tsize) {
    EvalShape s;
    s.HWs = HW <= 1024 ? (int)round_up(HW, 64) : HW;
    s.block = HW <= 1024 ? s.HWs : 1024;
    s.Ss = S / HW * s.HWs;
    s.lds = smem_layout(s.Ss, HWp, tsize, 2).total();
    s.improve_block = HW < 256 ? (int)round_up(HW, 64) : 256;
    s.improve_lds = S * tsize + (int)round_up(HWp, 16);
    return s;
}

constexpr unsigned long long kEvalNoError = ~0ull;  // the policy error word when every entry is in range

// A cell's policy lanes, packed as mgdp_vi_get_policy stores them: XYD 4 bytes (one per direction),
// DoorKey 16 bytes (lane l = (dir*2 + has_key)*2 + door_open).
struct Pk16 {
    uint32_t w[4];
};
template <int MODEL> struct PkOf { using type = uint32_t; };
template <> struct PkOf<MGDP_MODEL_DOORKEY> { using type = Pk16; };

// ------------------------------------------------------------------------------------------------
// The evaluation step of one cell: V'[s] = Q[s, pi(s)].  Deterministic: the value the chosen action
// reads is selected first, then multiplied once (fl(g * x), the table's R = 0 form); a terminal
// forward move takes its constant.  Slip: fl(p*Qd[pi(s)]) + xyd_slip_tail, the six-term chain.
// An absorbing state's lane is -1 (0xff): it falls to the self loop and is then zeroed.
// ------------------------------------------------------------------------------------------------
template <typename T, bool SLIP>
__device__ __forceinline__ T xyd_eval_step(const XydTopo<T> &tp, const Coef<T> &cf, const V4<T> &own,
                                           const T (&nbv)[4], uint32_t pk, V4<T> &out) {
    T dv = (T)0;
    if (!SLIP) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t a = (pk >> (8 * d)) & 0xffu;
            const T x = a == 0u ? own.v[(d + 3) & 3] : (a == 1u ? own.v[(d + 1) & 3] : (a == 2u ? nbv[d] : own.v[d]));
            T q = cf.g * x;
            q = (a == 2u && ((tp.term >> d) & 1u)) ? tp.tq[d] : q;
            const T best = tp.valid ? q : (T)0;
            out.v[d] = best;
            dv = vmax(dv, vabs(best - own.v[d]));
        }
        return dv;
    }
    T gv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) gv[d] = cf.g * own.v[d];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t a = (pk >> (8 * d)) & 0xffu;
        const T qF = xyd_forward<T, false, false>(tp, cf, d, nbv[d], (T)1);
        const T qL = gv[(d + 3) & 3], qR = gv[(d + 1) & 3], qS = gv[d];
        const T tail = xyd_slip_tail(cf, qL, qR, qF, qS);
        const T qa = a == 0u ? qL : (a == 1u ? qR : (a == 2u ? qF : qS));
        T best = cf.p * qa + tail;
        best = tp.valid ? best : (T)0;  // slip mixes in constants; absorbing states stay 0
        out.v[d] = best;
        dv = vmax(dv, vabs(best - own.v[d]));
    }
    return dv;
}

template <typename T>
__device__ __forceinline__ T dk_eval_step(const DkTopo &tp, const Coef<T> &cf, const T (&own)[16],
                                          const V4<T> (&nbs)[4], const Pk16 &pk, T (&outv)[16]) {
    T dv = (T)0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t f = tp.f[d];
        const V4<T> &nb = nbs[d];
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) {
#pragma unroll
            for (int dop = 0; dop < 2; ++dop) {
                const int l = (d * 2 + hk) * 2 + dop;
                const int hd = hk * 2 + dop;
                const uint32_t a = (pk.w[l >> 2] >> (8 * (l & 3))) & 0xffu;
                const T xS = own[l];
                const T xL = own[((d + 3) & 3) * 4 + hd];
                const T xR = own[((d + 1) & 3) * 4 + hd];
                T xM, xP, xT;
                dk_reads(f, hk, dop, own + d * 4, nb.v[hd], xM, xP, xT);
                const T x = a == 0u ? xL : (a == 1u ? xR : (a == 2u ? xM : (a == 3u ? xP : (a == 4u ? xT : xS))));
                T q = cf.g * x;
                if (a == 2u) q = dk_forward<T, false>(f, q, (T)1);
                const T best = ((tp.walk >> hd) & 1u) ? q : (T)0;
                outv[l] = best;
                dv = vmax(dv, vabs(best - own[l]));
            }
        }
    }
    return dv;
}

// One cell's sweep on the direction-major LDS tiles (stride HWs): own and front values from Vin,
// V' to Vout; returns the cell's max |dV|.
template <typename T, bool SLIP>
__device__ __forceinline__ T eval_cell(const XydTopo<T> &tp, uint32_t pk, const Coef<T> &cf, const T *Vin, T *Vout,
                                       int HWs, int c) {
    V4<T> own, out;
    T nbv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) own.v[d] = Vin[d * HWs + c];
    xyd_load_nb(tp, Vin, nbv);
    const T dv = xyd_eval_step<T, SLIP>(tp, cf, own, nbv, pk, out);
#pragma unroll
    for (int d = 0; d < 4; ++d) Vout[d * HWs + c] = out.v[d];
    return dv;
}
template <typename T, bool SLIP>
__device__ __forceinline__ T eval_cell(const DkTopo &tp, const Pk16 &pk, const Coef<T> &cf, const T *Vin, T *Vout,
                                       int HWs, int c) {
    T own[16], outv[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const V4<T> x = *reinterpret_cast<const V4<T> *>(Vin + (q * HWs + c) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) own[4 * q + j] = x.v[j];
    }
    V4<T> nbs[4];
    dk_load_nb(tp, Vin, nbs);
    const T dv = dk_eval_step<T>(tp, cf, own, nbs, pk, outv);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<V4<T> *>(Vout + (q * HWs + c) * 4) =
            V4<T>{{outv[4 * q], outv[4 * q + 1], outv[4 * q + 2], outv[4 * q + 3]}};
    return dv;
}

template <typename T>
__device__ __forceinline__ XydTopo<T> eval_topo(const uint8_t *cl, const Geo &geo, int c, XydTopo<T> *) {
    return xyd_topo_soa<T>(cl, geo, c);
}
template <typename T>
__device__ __forceinline__ DkTopo eval_topo(const uint8_t *cl, const Geo &geo, int c, DkTopo *) {
    return dk_topo_soa(cl, geo, c);
}

// A cell's lanes as given -> as stored: absorbing states -1.  A lane outside [0, A) on a valid state
// sets `bad` and folds {grid, state, action} into the error word (the minimum: the first offending
// grid, and its first offending state).
template <typename T>
__device__ __forceinline__ uint32_t resolve_pi(const XydTopo<T> &tp, const int8_t *src, int8_t *dst, int c, int e,
                                               unsigned long long *everr, bool &bad) {
    uint32_t pk = *reinterpret_cast<const uint32_t *>(src + c * 4);
    if (!tp.valid) pk = 0xffffffffu;
#pragma unroll
    for (int d = 3; d >= 0; --d) {
        const uint32_t a = (pk >> (8 * d)) & 0xffu;
        if (tp.valid && a >= 7u) {
            bad = true;
            atomicMin(everr, ((unsigned long long)e << 32) | ((unsigned long long)(c * 4 + d) << 8) | a);
        }
    }
    *reinterpret_cast<uint32_t *>(dst + c * 4) = pk;
    return pk;
}
__device__ __forceinline__ Pk16 resolve_pi(const DkTopo &tp, const int8_t *src, int8_t *dst, int c, int e,
                                           unsigned long long *everr, bool &bad) {
    const uint4 raw = *reinterpret_cast<const uint4 *>(src + c * 16);
    Pk16 pk = {{raw.x, raw.y, raw.z, raw.w}};
#pragma unroll
    for (int l = 15; l >= 0; --l) {
        const bool valid = (tp.walk >> (l & 3)) & 1u;  // l & 3 = has_key*2 + door_open
        if (!valid) pk.w[l >> 2] |= 0xffu << (8 * (l & 3));
        const uint32_t a = (pk.w[l >> 2] >> (8 * (l & 3))) & 0xffu;
        if (valid && a >= 5u) {
            bad = true;
            atomicMin(everr, ((unsigned long long)e << 32) | ((unsigned long long)(c * 16 + l) << 8) | a);
        }
    }
    *reinterpret_cast<uint4 *>(dst + c * 16) = make_uint4(pk.w[0], pk.w[1], pk.w[2], pk.w[3]);
    return pk;
}

// HBM row (cell-major, the ABI's order) <-> direction-major LDS tile, one cell
template <typename T, int MODEL>
__device__ __forceinline__ void eval_load_cell(T *tile, const T *Vg, int HWs, int c) {
    if constexpr (MODEL == MGDP_MODEL_XYD) {
        const V4<T> x = *reinterpret_cast<const V4<T> *>(Vg + c * 4);
#pragma unroll
        for (int d = 0; d < 4; ++d) tile[d * HWs + c] = x.v[d];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<V4<T> *>(tile + (q * HWs + c) * 4) = *reinterpret_cast<const V4<T> *>(Vg + c * 16 + 4 * q);
    }
}
template <typename T, int MODEL>
__device__ __forceinline__ void eval_store_cell(T *Vg, const T *tile, int HWs, int c) {
    if constexpr (MODEL == MGDP_MODEL_XYD) {
        V4<T> x;
#pragma unroll
        for (int d = 0; d < 4; ++d) x.v[d] = tile[d * HWs + c];
        *reinterpret_cast<V4<T> *>(Vg + c * 4) = x;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<V4<T> *>(Vg + c * 16 + 4 * q) = *reinterpret_cast<const V4<T> *>(tile + (q * HWs + c) * 4);
    }
}

// ------------------------------------------------------------------------------------------------
// Policy evaluation, one workgroup per grid: cells, the packed policy and both V tiles stay in LDS for
// the whole evaluation (HBM: one read of cells and pi, one write of V and of the normalised pi; nothing
// per sweep).  The fused protocol unchanged: k_target < 0 runs the grid's own rule (stop after the
// sweep whose max|dV| < tol, or at max_sweeps), else exactly to k_target with |dV| of the last sweep;
// fresh starts from V_0 = 0, else from kenv / dvenv and V in HBM; a grid at an exact fixed point is
// complete for any later k_target.  The launch resolves pi_src (which may be the handle's own pi
// buffer) into pi when fresh; a grid with a lane out of range sweeps nothing and reports sweep 0.
// With W*H <= blockDim a thread keeps its cell's topology and lanes in registers; above, the cells are
// strided over the workgroup and both are re-read from LDS every sweep.
// ------------------------------------------------------------------------------------------------
template <typename T, int MODEL, bool SLIP>
__global__ void __launch_bounds__(1024)
vi_eval_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, T *__restrict__ V, const int8_t *pi_src,
               int8_t *pi, int32_t *__restrict__ kenv, double *__restrict__ dvenv,
               unsigned long long *__restrict__ red, unsigned int *__restrict__ ticket,
               unsigned long long *__restrict__ host_out, unsigned long long *__restrict__ everr, int k_target,
               int fresh, int in_kernel_reduce, unsigned int epoch) {
    using Topo = typename TopoOf<T, MODEL>::type;
    using Pk = typename PkOf<MODEL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem L = smem_layout(geo.Ss, geo.HWp, (int)sizeof(T), 2);
    T *V0 = reinterpret_cast<T *>(smem);
    T *V1 = reinterpret_cast<T *>(smem + L.v_bytes);
    Pk *pis = reinterpret_cast<Pk *>(smem + L.pi_off());
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + L.cells_off());
    T *slots = reinterpret_cast<T *>(smem + L.slots_off());
    uint8_t *flags = reinterpret_cast<uint8_t *>(smem + L.flags_off());
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, HW = geo.HW, HWs = geo.HWs;
    int k = fresh ? 0 : kenv[e];
    double dvl = fresh ? 0.0 : dvenv[e];
    if (k_target > k && k > 0 && dvl == 0.0) {  // fixed-point completion (grid_complete_at)
        if (tid == 0) kenv[e] = k_target;
        k = k_target;
    }
    const bool own_rule = k_target < 0;
    // (grid_has_work, written out: the shared predicates moved this kernel's registers)
    const bool work = own_rule ? (!(k > 0 && dvl < geo.tol) && k < geo.max_sweeps) : (k < k_target);
    if (work) {
        const long long vb = (long long)e * geo.S;
        T *Vg = V + vb;
        copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
        if (tid < 64) flags[tid] = 0;
        if (k == 0) {
            zero16(V0, 2 * L.v_bytes);
        } else {
            for (int c = tid; c < HW; c += nt) eval_load_cell<T, MODEL>(V0, Vg, HWs, c);
        }
        __syncthreads();
        const bool reg = HW <= nt;
        Topo tp = {};
        Pk pk = {};
        bool bad = false;
        if (reg) {
            if (tid < HW) {
                tp = eval_topo<T>(cl, geo, tid, (Topo *)nullptr);
                if (fresh) pk = resolve_pi(tp, pi_src + vb, pi + vb, tid, e, everr, bad);
                else pk = *reinterpret_cast<const Pk *>(pi + vb + (long long)tid * sizeof(Pk));
            }
        } else {
            for (int c = tid; c < HW; c += nt) {
                const Topo t = eval_topo<T>(cl, geo, c, (Topo *)nullptr);
                if (fresh) pis[c] = resolve_pi(t, pi_src + vb, pi + vb, c, e, everr, bad);
                else pis[c] = *reinterpret_cast<const Pk *>(pi + vb + (long long)c * sizeof(Pk));
            }
        }
        // (also the barrier after which the strided lanes are read; flag parity 1: the first sweep
        // writes parity 0, and parity 1 is rewritten only after the first sweep's barrier)
        if (block_any(bad, flags, 1)) {
            k = 0;
            dvl = 0.0;
        } else {
            T *Vin = V0, *Vout = V1;
            int parity = 0;
            T diff = (T)0;
            while (own_rule ? k < geo.max_sweeps : k < k_target) {
                T d = (T)0;
                if (reg) {
                    if (tid < HW) d = eval_cell<T, SLIP>(tp, pk, cf, Vin, Vout, HWs, tid);
                } else {
                    for (int c = tid; c < HW; c += nt)
                        d = vmax(d, eval_cell<T, SLIP>(eval_topo<T>(cl, geo, c, (Topo *)nullptr), pis[c], cf, Vin, Vout, HWs, c));
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
            for (int c = tid; c < HW; c += nt) eval_store_cell<T, MODEL>(Vg, Vin, HWs, c);
        }
        record_grid(geo, kenv, dvenv, e, k, dvl, tid == 0);
    }
    if (in_kernel_reduce)
        fused_reduce(red, ticket, host_out, k, dvl, reinterpret_cast<unsigned int *>(slots + 16), epoch, false, tid);
}

// ------------------------------------------------------------------------------------------------
// Greedy improvement: pi'(s) = argmax_a Q(s, a) on V, lowest action index among exact maxima, except
// that pi(s) stays when Q(s, pi(s)) equals the maximum (so "no state changed" is a valid stop of policy
// iteration).  Q is xyd_mix / dk_q5 (vi_model.h), the values xyd_step / dk_step maximise.  Returns the
// packed new lanes and adds the changed valid states to n.  A current lane outside [0, A) never keeps.
// ND: the NoDeath Q -- the move into lava carries dc; Q may be negative, and the
// comparisons are plain either way.
// ------------------------------------------------------------------------------------------------
template <typename T, bool SLIP, bool ND>
__device__ __forceinline__ uint32_t xyd_improve_step(const XydTopo<T> &tp, const Coef<T> &cf, const V4<T> &own,
                                                     const T (&nbv)[4], uint32_t old, unsigned int &n) {
    T gv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) gv[d] = cf.g * own.v[d];
    uint32_t pk = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        T q[4];
        xyd_mix<T, SLIP>(cf, gv[(d + 3) & 3], gv[(d + 1) & 3], xyd_forward<T, ND, false>(tp, cf, d, nbv[d], (T)1), gv[d], q);
        uint32_t arg;
        const T best = q_argmax(q, arg);
        const uint32_t cur = (old >> (8 * d)) & 0xffu;
        const T qc = cur == 0u ? q[0] : (cur == 1u ? q[1] : (cur == 2u ? q[2] : q[3]));
        if (cur < 7u && qc == best) arg = cur;
        if (tp.valid && arg != cur) ++n;
        pk |= (tp.valid ? arg : 0xffu) << (8 * d);
    }
    return pk;
}

template <typename T>
__device__ __forceinline__ Pk16 dk_improve_step(const DkTopo &tp, const Coef<T> &cf, const T (&own)[16],
                                                const V4<T> (&nbs)[4], const Pk16 &old, unsigned int &n) {
    T gv[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) gv[l] = cf.g * own[l];
    Pk16 pk = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t f = tp.f[d];
        const V4<T> &nb = nbs[d];
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) {
#pragma unroll
            for (int dop = 0; dop < 2; ++dop) {
                const int l = (d * 2 + hk) * 2 + dop;
                const int hd = hk * 2 + dop;
                T q[5];
                dk_q5(f, hk, dop, gv[((d + 3) & 3) * 4 + hd], gv[((d + 1) & 3) * 4 + hd], gv + d * 4, cf.g * nb.v[hd], q);
                const bool valid = (tp.walk >> hd) & 1u;
                uint32_t arg;
                const T best = q_argmax(q, arg);
                const uint32_t cur = (old.w[l >> 2] >> (8 * (l & 3))) & 0xffu;
                const T qc = cur == 0u ? q[0] : (cur == 1u ? q[1] : (cur == 2u ? q[2] : (cur == 3u ? q[3] : q[4])));
                if (cur < 5u && qc == best) arg = cur;
                if (valid && arg != cur) ++n;
                pk.w[l >> 2] |= (valid ? arg : 0xffu) << (8 * (l & 3));
            }
        }
    }
    return pk;
}

// One pass per grid over the V in HBM: the grid's V row (cell-major) and cells are staged into LDS,
// each thread improves its cells' lanes in place in pi, and the workgroup adds its count of changed
// states to *changed (one vector atomic per workgroup that changed anything).  ND (XYD only): the
// NoDeath topology and Q.
template <typename T, int MODEL, bool SLIP, bool ND>
__global__ void __launch_bounds__(256)
vi_improve_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, const T *__restrict__ V,
                  int8_t *__restrict__ pi, unsigned long long *__restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned int cnt;
    T *Vs = reinterpret_cast<T *>(smem);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + geo.S * (int)sizeof(T));
    const int e = blockIdx.x;
    const long long vb = (long long)e * geo.S;
    copy16(Vs, V + vb, geo.S * (int)sizeof(T));
    copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    unsigned int n = 0;
    for (int c = threadIdx.x; c < geo.HW; c += blockDim.x) {
        if constexpr (MODEL == MGDP_MODEL_XYD) {
            const XydTopo<T> tp = xyd_topo<T, ND>(cl, geo, c);
            const V4<T> own = *reinterpret_cast<const V4<T> *>(Vs + c * 4);
            T nbv[4];
            xyd_load_nb(tp, Vs, nbv);
            uint32_t *p = reinterpret_cast<uint32_t *>(pi + vb + c * 4);
            *p = xyd_improve_step<T, SLIP, ND>(tp, cf, own, nbv, *p, n);
        } else {
            const DkTopo tp = dk_topo(cl, geo, c);
            T own[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const V4<T> x = *reinterpret_cast<const V4<T> *>(Vs + c * 16 + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) own[4 * q + j] = x.v[j];
            }
            V4<T> nbs[4];
            dk_load_nb(tp, Vs, nbs);
            uint4 *p = reinterpret_cast<uint4 *>(pi + vb + c * 16);
            const uint4 o = *p;
            const Pk16 nw = dk_improve_step<T>(tp, cf, own, nbs, Pk16{{o.x, o.y, o.z, o.w}}, n);
            *p = make_uint4(nw.w[0], nw.w[1], nw.w[2], nw.w[3]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&cnt, n);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(changed, (unsigned long long)cnt);
}

}  // namespace mgdp
