// vi_qvalues.h -- the action values of the handle's V: Q[B][S][A] and the set of
// maximising actions per state, opt[B][S] (bit a: Q[s,a] equals the row's maximum in T).  One pass per grid
// over the V in HBM, staged as vi_improve_kernel stages it; the values are the ones its argmax compares,
// from the same definitions (vi_model.h: xyd_forward / xyd_mix, dk_q5, q_argmax):
//     Qd[s,a] = done ? R : fl(R + fl(g*V[s']))       (R = 0 where not done; NoDeath lava: R = dc)
//     Q[s,a]  = Qd[s,a]                               deterministic
//     Q[s,a]  = fl(fl(p*Qd[s,a]) + fl(c*s6))          slip, s6 = ((((Qd0+Qd1)+Qd2)+Qd3)+Qd4)+Qd5
// Walls and absorbing states hold +0 in every lane and opt 0.  Part of the single translation unit vi.hip
// (included after vi_eval.h).
#pragma once

namespace mgdp {

// A work item is what one lane computes: a cell of the XYD model (4 states x 7 actions) or one direction of
// a DoorKey cell (4 states x 5 actions).  Item i of a grid owns the values [i*kVals, (i+1)*kVals) of the
// grid's Q row and the opt bytes [4i, 4i+4): a wave's 64 items are one contiguous piece of both.
constexpr int q_item_vals(int model) { return 4 * (model == MGDP_MODEL_XYD ? 7 : 5); }  // 28 / 20
constexpr int q_item_bytes(int model, int tsize) { return q_item_vals(model) * tsize; }  // 112, 224 / 80, 160: a multiple of 16
// The staging stride of an item.  ds_write_b128 is served in groups of 8 consecutive lanes on 32 banks: at 28
// or 20 dwords the 8 lanes start on 8 different multiples of 4 banks (no conflict); at 56 or 40 dwords (fp64)
// lanes l and l+4 share theirs, so fp64 items are 16 bytes apart (60 / 44 dwords).
constexpr int q_item_stride(int model, int tsize) { return q_item_bytes(model, tsize) + (tsize == 8 ? 16 : 0); }
template <typename T, int MODEL>
struct QItem {
    static constexpr int kVals = q_item_vals(MODEL);
    static constexpr int kBytes = q_item_bytes(MODEL, (int)sizeof(T));
    static constexpr int kSlots = kBytes / 16;  // 16-byte pieces of an item
    static constexpr int kStride = q_item_stride(MODEL, (int)sizeof(T));
    static constexpr int kWaveBytes = 64 * kStride;  // a wave's staging area
};
inline int qvalues_block(int model, int HW) {
    const int items = model == MGDP_MODEL_XYD ? HW : 4 * HW;
    return items < 256 ? (int)round_up(items, 64) : 256;
}
// LDS: [V row, cell-major][cells][a staging area per wave]
inline int qvalues_lds(int model, int HW, int HWp, int S, int tsize, bool write_q) {
    const int base = S * tsize + (int)round_up(HWp, 16);
    return base + (write_q ? qvalues_block(model, HW) * q_item_stride(model, tsize) : 0);
}

template <typename T>
__device__ __forceinline__ uint32_t q_opt_bit(T q, T m, uint32_t bits) { return q == m ? bits : 0u; }

// The 28 values and 4 opt bytes of an XYD cell: the values xyd_improve_step compares.
template <typename T, bool SLIP, bool ND>
__device__ __forceinline__ uint32_t xyd_q_step(const XydTopo<T> &tp, const Coef<T> &cf, const V4<T> &own,
                                               const T (&nbv)[4], T (&q)[28]) {
    T gv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) gv[d] = cf.g * own.v[d];
    uint32_t opt = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        T a[4];  // Q of actions 0..3 (4..6 equal action 3)
        xyd_mix<T, SLIP>(cf, gv[(d + 3) & 3], gv[(d + 1) & 3], xyd_forward<T, ND, false>(tp, cf, d, nbv[d], (T)1), gv[d], a);
        int arg;
        const T best = q_argmax(a, arg);
        const uint32_t bits = q_opt_bit(a[0], best, 1u) | q_opt_bit(a[1], best, 2u) | q_opt_bit(a[2], best, 4u) | q_opt_bit(a[3], best, 0x78u);
        opt |= (tp.valid ? bits : 0u) << (8 * d);
#pragma unroll
        for (int i = 0; i < 7; ++i) q[7 * d + i] = tp.valid ? a[i < 3 ? i : 3] : (T)0;
    }
    return opt;
}

// The 20 values and 4 opt bytes of direction d of a DoorKey cell (states l = d*4 + has_key*2 + door_open): the
// values dk_improve_step compares.  ownD / ownL / ownR: the cell's V of direction d, d-1, d+1; nb: the
// front cell's V of direction d; f: DkTopo::f[d].
template <typename T>
__device__ __forceinline__ uint32_t dk_q_step(uint32_t walk, uint32_t f, const Coef<T> &cf, const V4<T> &ownD,
                                              const V4<T> &ownL, const V4<T> &ownR, const V4<T> &nb, T (&q)[20]) {
    T gD[4], gL[4], gR[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gD[j] = cf.g * ownD.v[j];
        gL[j] = cf.g * ownL.v[j];
        gR[j] = cf.g * ownR.v[j];
    }
    uint32_t opt = 0;
#pragma unroll
    for (int hk = 0; hk < 2; ++hk) {
#pragma unroll
        for (int dop = 0; dop < 2; ++dop) {
            const int hd = hk * 2 + dop;
            T a[5];
            dk_q5(f, hk, dop, gL[hd], gR[hd], gD, cf.g * nb.v[hd], a);
            const bool valid = (walk >> hd) & 1u;
            int arg;
            const T best = q_argmax(a, arg);
            uint32_t bits = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                bits |= q_opt_bit(a[i], best, 1u << i);
                q[5 * hd + i] = valid ? a[i] : (T)0;
            }
            opt |= (valid ? bits : 0u) << (8 * hd);
        }
    }
    return opt;
}

// One workgroup per grid; the grid's V row (cell-major) and cells are staged into LDS, every lane computes
// an item per pass, and opt goes out as one dword per lane (a wave: 256 contiguous bytes).  Q goes through
// the wave's own staging area: every lane writes its item with 16-byte LDS stores, then the wave writes its
// contiguous piece of the Q row with 16-byte global stores, consecutive lanes on consecutive addresses --
// stored from the lanes directly, one store instruction would touch 64 pieces 80 to 224 bytes apart.  The
// staging area is private to the wave, so the two sides are ordered by wave-level fences, not a barrier.
// Q or opt may be null (workgroup-uniform); all offsets into Q are 64-bit.
template <typename T, int MODEL, bool SLIP, bool ND>
__global__ void __launch_bounds__(256)
vi_qvalues_kernel(Geo geo, Coef<T> cf, const uint8_t *__restrict__ cells, const T *__restrict__ V, T *__restrict__ Q,
                  uint8_t *__restrict__ opt) {
    using I = QItem<T, MODEL>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *Vs = reinterpret_cast<T *>(smem);
    uint8_t *cl = reinterpret_cast<uint8_t *>(smem + geo.S * (int)sizeof(T));
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned char *stage = smem + geo.S * (int)sizeof(T) + (int)round_up(geo.HWp, 16) + wave * I::kWaveBytes;
    const long long vb = (long long)e * geo.S;
    copy16(Vs, V + vb, geo.S * (int)sizeof(T));
    copy16(cl, cells + (long long)e * geo.HWp, geo.HWp);
    __syncthreads();
    const int items = MODEL == MGDP_MODEL_XYD ? geo.HW : 4 * geo.HW;
    unsigned char *Qg = reinterpret_cast<unsigned char *>(Q) + vb * I::kBytes / 4;  // S*A*sizeof(T) = S/4 items per grid
    for (int base = wave * 64; base < items; base += (int)blockDim.x) {
        const int it = base + lane;
        T q[I::kVals];
        uint32_t ob = 0;
        if (it < items) {
            if constexpr (MODEL == MGDP_MODEL_XYD) {
                const XydTopo<T> tp = xyd_topo<T, ND>(cl, geo, it);
                const V4<T> own = *reinterpret_cast<const V4<T> *>(Vs + it * 4);
                T nbv[4];
                xyd_load_nb(tp, Vs, nbv);
                ob = xyd_q_step<T, SLIP, ND>(tp, cf, own, nbv, q);
            } else {
                const int c = it >> 2, d = it & 3;
                const DkTopo tp = dk_topo(cl, geo, c);
                const uint32_t f = d == 0 ? tp.f[0] : (d == 1 ? tp.f[1] : (d == 2 ? tp.f[2] : tp.f[3]));
                const int nbi = d == 0 ? tp.nb[0] : (d == 1 ? tp.nb[1] : (d == 2 ? tp.nb[2] : tp.nb[3]));
                const V4<T> ownD = *reinterpret_cast<const V4<T> *>(Vs + c * 16 + d * 4);
                const V4<T> ownL = *reinterpret_cast<const V4<T> *>(Vs + c * 16 + ((d + 3) & 3) * 4);
                const V4<T> ownR = *reinterpret_cast<const V4<T> *>(Vs + c * 16 + ((d + 1) & 3) * 4);
                const V4<T> nb = *reinterpret_cast<const V4<T> *>(Vs + nbi);
                ob = dk_q_step<T>(tp.walk, f, cf, ownD, ownL, ownR, nb, q);
            }
            if (opt) *reinterpret_cast<uint32_t *>(opt + vb + (long long)it * 4) = ob;
        }
        if (Q) {
            if (it < items) {
                constexpr int per = 16 / (int)sizeof(T);  // values per 16-byte piece
#pragma unroll
                for (int j = 0; j < I::kSlots; ++j) {
                    uint4 w;
                    if constexpr (sizeof(T) == 4) {
                        w = make_uint4(__float_as_uint(q[4 * j]), __float_as_uint(q[4 * j + 1]), __float_as_uint(q[4 * j + 2]),
                                       __float_as_uint(q[4 * j + 3]));
                    } else {
                        const unsigned long long a = (unsigned long long)__double_as_longlong(q[per * j]);
                        const unsigned long long b = (unsigned long long)__double_as_longlong(q[per * j + 1]);
                        w = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
                    }
                    *reinterpret_cast<uint4 *>(stage + lane * I::kStride + j * 16) = w;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int n = items - base < 64 ? items - base : 64;  // the wave's items of this pass
            const int nslots = n * I::kSlots;
            unsigned char *dst = Qg + (long long)base * I::kBytes;
#pragma unroll
            for (int j = 0; j < I::kSlots; ++j) {
                const int slot = j * 64 + lane;
                if (slot < nslots) {
                    const int item = slot / I::kSlots, w = slot - item * I::kSlots;
                    *reinterpret_cast<uint4 *>(dst + (long long)slot * 16) =
                        *reinterpret_cast<const uint4 *>(stage + item * I::kStride + w * 16);
                }
            }
            // the next pass rewrites the staging area: its reads above come first
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

}  // namespace mgdp
