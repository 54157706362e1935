// vi_layout.h -- sizes of the value-iteration kernels' LDS and device buffers: the one definition
// the host's plan (vi_plan.h) and the device loops (vi_loops.h, vi_kernels.h) both use.  Plain
// C++17: MGDP_HD is __host__ __device__ under hipcc and empty for a host compiler.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGDP_HD __host__ __device__
#else
#define MGDP_HD
#endif

namespace mgdp {

MGDP_HD inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

constexpr int kInKernelReduceMaxB = 512;  // above this, a separate one-workgroup reduce kernel
constexpr int kBreqCopies = 64;           // batch server: request lines (workgroup w polls w % copies)

// The usual fused layout: [nbuf V tiles][pi][cells][block_max slots 256 B][flags 64 B]
struct Smem {
    int nbuf, v_bytes, pi_bytes, cells_bytes, slot_bytes;
    MGDP_HD int total() const { return nbuf * v_bytes + pi_bytes + cells_bytes + slot_bytes; }
    MGDP_HD int pi_off() const { return nbuf * v_bytes; }
    MGDP_HD int cells_off() const { return nbuf * v_bytes + pi_bytes; }
    MGDP_HD int slots_off() const { return nbuf * v_bytes + pi_bytes + cells_bytes; }
    MGDP_HD int flags_off() const { return slots_off() + 256; }
};

MGDP_HD inline Smem smem_layout(int S, int HWp, int tsize, int nbuf = 2) {
    Smem m;
    m.nbuf = nbuf;
    m.v_bytes = S * tsize;  // S is a multiple of 4 -> 16-B multiple for f32, f64
    m.pi_bytes = (S + 15) / 16 * 16;
    m.cells_bytes = HWp;
    m.slot_bytes = 256 + 64;  // block_max slots [2][16] x 8 B + convergence flags [2][2][16] B
    return m;
}

// fused_serve_xyd: each tile = [pad][plane 1][pad][plane 3][pad], carved from the two V buffers
MGDP_HD inline int serve_ew_padw(int W) { return (W + 15) / 16 * 16; }
MGDP_HD inline int serve_ew_tile_elems(int HWs, int W) { return 2 * HWs + 3 * serve_ew_padw(W); }
// fused_serve_pair: two cell-major tiles, each [pad][HWs][pad] cells of four planes side by side (16 B for
// fp32), pad = round_up(2W, 16) cells; serve_pair_plane is a tile's cells, with the pads
MGDP_HD inline int serve_pair_pad(int W) { return (2 * W + 15) / 16 * 16; }
MGDP_HD inline int serve_pair_plane(int HWs, int W) { return HWs + 2 * serve_pair_pad(W); }
MGDP_HD inline int serve_pair_tile_elems(int HWs, int W) { return 4 * serve_pair_plane(HWs, W); }

// fused_wave2_xyd: [slots 256 B][cells HWp][tile: pad | plane 3 (64P) | plane 1 (64P) | pad]
MGDP_HD inline int wave2_padw(int W) { return (W + 15) / 16 * 16; }
MGDP_HD inline int wave2_tile_off(int HWp) { return 256 + (HWp + 15) / 16 * 16; }
MGDP_HD inline int wave2_smem_bytes(int HWp, int W, int P, int tsize) {
    return wave2_tile_off(HWp) + (2 * 64 * P + 2 * wave2_padw(W)) * tsize;
}
// fused_band_xyd: [slots 256 B][cells HWp], no tile; HB = rows per column band
MGDP_HD inline int band_rows(int W, int H) { return W > 64 ? 0 : (H + 64 / W - 1) / (64 / W); }
MGDP_HD inline int band_smem_bytes(int HWp) { return wave2_tile_off(HWp); }
// fused_wave2n_xyd: [slots 256 B][cells HWp][tile 0][tile 1][edges 4 T | dV 2 T | flags 4 u32]
MGDP_HD inline int wave2n_tile_elems(int W, int P) { return 2 * 64 * P + 2 * wave2_padw(W); }
MGDP_HD inline int wave2n_smem_bytes(int HWp, int W, int P, int tsize) {
    return wave2_tile_off(HWp) + 2 * wave2n_tile_elems(W, P) * tsize + 64;
}
// A mixed launch (Loop::mix): P blocks on one wave or 2 * ceil(P / 2) on two, the larger layout
MGDP_HD inline int mix_smem_bytes(int HWp, int W, int P, int tsize) {
    const int a = wave2_smem_bytes(HWp, W, P, tsize), b = wave2n_smem_bytes(HWp, W, 2 * ((P + 1) / 2), tsize);
    return a > b ? a : b;
}

// The in-launch reduction's device words (GkCtx, vi_loops.h): counters, shard slots, grid slots
constexpr int kGkShards = 256;
constexpr int kGkLine = 16;                                    // u64 words per 128-B line
constexpr int kGkCnt2 = 0;                                     // [256 shard counter lines][top line]
constexpr int kGkTop2 = kGkCnt2 + kGkShards * kGkLine;
constexpr int kGkSxMin = kGkTop2 + kGkLine;                    // int32 [256] shard min reported sweeps
constexpr int kGkSxMax = kGkSxMin + kGkShards / 2;             // int32 [256] shard max reported sweeps
constexpr int kGkSxDv = kGkSxMax + kGkShards / 2;              // u64 [256] shard max dV bits
MGDP_HD inline int gk_kr_off(int B) { (void)B; return kGkSxDv + kGkShards; }  // int32 [B] sweeps,
MGDP_HD inline int gk_dv_off(int B) { return gk_kr_off(B) + (B + 1) / 2; }     // u64 [B] dV bits
MGDP_HD inline int gk_kn_off(int B) { return gk_dv_off(B) + B; }               // int32 [B] min sweeps (KMIN)
MGDP_HD inline int gk_words(int B) { return gk_kn_off(B) + (B + 1) / 2; }

// fused_dk_rows: [slots 256][flags 64][row map 128][cells HWp][tile 0: plane 1 | plane 3][tile 1: ...],
// each plane PL = HWs + 32 V4 entries
MGDP_HD inline int dkrow_cells_off() { return 256 + 64 + 128; }
MGDP_HD inline int dkrow_tile_off(int HWp) { return dkrow_cells_off() + (HWp + 15) / 16 * 16; }
MGDP_HD inline int dkrow_plane(int HWs) { return HWs + 32; }  // V4 entries per plane
MGDP_HD inline int dkrow_smem_bytes(int HWp, int HWs, int tsize) {
    return dkrow_tile_off(HWp) + 2 * 2 * dkrow_plane(HWs) * 4 * tsize;
}

// vi_sweep_kernel (m grids staged per iteration) and vi_sweep_pipe_kernel
MGDP_HD inline int sweep_smem_bytes(int S, int HWp, int tsize, int m) {
    return 2 * m * S * tsize + m * ((S + 15) / 16 * 16) + m * HWp + 256;
}
MGDP_HD inline int sweep_pipe_smem_bytes(int S, int HW, int HWs, int HWp, int tsize) {
    return S / HW * HWs * tsize + HWp + 256;
}

}  // namespace mgdp
