// recon_pieces.h - the pieces a block item of the reconstruction kernel (recon_kernel.hip, tx_item) says once: the item's geometry, the
// walk over a block's rows in 16-byte pieces with the copies between frame rows and LDS tiles built on it, and the dispatch over the
// pruned inverse networks.  Device only; everything is inlined into the item.
#ifndef AV1MI_RECON_PIECES_H
#define AV1MI_RECON_PIECES_H
#include <stdint.h>

#define AV1MI_RP_FN static __device__ __forceinline__

namespace av1mi_recon {

// Geometry of an item: a transform block of N = 1 << LOG2N samples a side per lane group, NPL groups to the wave.  (The per-group offset
// inside the edge arrays, EDGO, is not here: it is the edge arrays' size, which belongs to the LDS layout in recon_kernel.hip.)
template <int LOG2N_, int NPL>
struct ItemGeom {
  static constexpr int LOG2N = LOG2N_, N = 1 << LOG2N;
  static constexpr int ST = N + 1;        // row stride of the transform passes' staging tile
  // MM: luma 32x32 blocks run the forward transform as a matrix product on the matrix cores: the residual rows are
  // then read with 128-bit loads, so they lie 32 apart (16-byte aligned) instead of 33
  static constexpr bool MM = LOG2N == 5 && NPL == 1;
  // VEC: block classes whose DC / V / H prediction and residual are written eight samples per lane and step (128-bit LDS accesses):
  // luma 32x32 and the chroma 16x16 pair; their residual rows lie 32 / 24 apart (16-byte aligned)
  static constexpr bool VEC = MM || (LOG2N == 4 && NPL == 2);
  static constexpr int STR = MM ? 32 : (VEC ? 24 : ST);   // row stride of the residual
  static constexpr int G = 64 / NPL;      // lanes per group
  static constexpr int PIXO = NPL == 1 ? 0 : (N > 16 ? 1024 : 512);   // per-group offset inside srcblk / blkpix (NPL == 2: N <= 16, or 32 in the 64x64 build)
  static constexpr int SCRO = NPL == 1 ? 0 : (N > 16 ? 32 * 33 : 16 * 24);   // ... inside scratch (16 rows of stride 24: see STR)
  static constexpr int EB = 8;            // index of element 0 inside a group's edge array
  // PVOK: block classes with the piece-wise intra predictors (eight samples of a row per lane and step; intra_pieces.h)
  static constexpr bool PVOK = N >= 8;
  // 64-point transforms (64x64 build): only the 32x32 low-frequency corner is coded (CW = 32) - the column pass keeps its first
  // 32 outputs, the row pass runs on 32 lanes and keeps 32, the inverse passes take 32 inputs (zeros beyond) and give 64 outputs
  static constexpr int CW = N > 32 ? 32 : N;
  // shifts of the forward passes (input, between the passes, before the quantiser) and of the inverse row pass
  static constexpr int SH0 = LOG2N == 6 ? 0 : 2, SH1 = LOG2N == 2 ? 0 : (LOG2N == 3 ? 1 : (LOG2N == 4 ? 2 : (LOG2N == 5 ? 4 : 2))), SH2 = LOG2N == 6 ? 2 : 0;
  static constexpr int RS = LOG2N == 2 ? 0 : (LOG2N == 3 ? 1 : 2);
  static constexpr int TSH = LOG2N == 6 ? 2 : (LOG2N == 5 ? 1 : 0);   // dequant shift of the size class (§7.12.3)
};

typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef u4 u4_any __attribute__((aligned(2)));   // 16 bytes at any 2-byte alignment

// ---- a block's rows in 16-byte pieces, PER of them to a row: lane sl of a group of G lanes takes the pieces sl, sl + G, ... and calls
// f(row, piece of that row)
template <int N, int PER, int G, typename F>
AV1MI_RP_FN void for_row_pieces(int sl, F f) {
#pragma unroll
  for (int q = sl; q < N * PER; q += G) { const int r = q / PER; f(r, q - r * PER); }
}
// a block of PIX samples moves in 16-byte pieces where its rows hold whole pieces that are 16-byte aligned in the frame (stride gs,
// first column gx) and lie inside the frame: 8 samples of 16 bits, 16 of 8
template <typename PIX, int N> struct RowPieces { static constexpr int SPP = 16 / (int)sizeof(PIX); static constexpr bool OK = N >= SPP; };
template <typename PIX>
AV1MI_RP_FN bool rows_aligned(bool overhang, int gs, int gx) { return !overhang && ((gs | gx) & (16 / (int)sizeof(PIX) - 1)) == 0; }

// 16-bit rows (stride `stride` samples, ALIGNED: on 16-byte boundaries) from HBM -> tile of N x N.  Every load before the first LDS store -
// in one loop the compiler keeps source order, load -> wait -> store -> load ...: a memory round trip per piece; the loads unconditional,
// the index clamped: a load under a condition is waited for on the spot.
template <int N, int G, bool ALIGNED = true>
AV1MI_RP_FN void rows_to_tile(int sl, const uint16_t *src, int stride, uint16_t *tile) {
  constexpr int CPR = N / 8, CNT = (N * CPR + G - 1) / G;
  u4 v[CNT];
#pragma unroll
  for (int k = 0; k < CNT; k++) {
    const int q = sl + k * G < N * CPR ? sl + k * G : 0, r = q / CPR, c8 = q - r * CPR;
    const uint16_t *p = src + (size_t)r * stride + 8 * c8;
    v[k] = ALIGNED ? *reinterpret_cast<const u4 *>(p) : *reinterpret_cast<const u4_any *>(p);
  }
#pragma unroll
  for (int k = 0; k < CNT; k++) {
    const int q = sl + k * G, r = q / CPR, c8 = q - r * CPR;
    if (q < N * CPR) *reinterpret_cast<u4 *>(tile + r * N + 8 * c8) = v[k];
  }
}
// ... 8-bit rows, 16 samples per load (always on 16-byte boundaries), widened to the tile's 16-bit layout
template <int N, int G>
AV1MI_RP_FN void rows_to_tile(int sl, const uint8_t *src, int stride, uint16_t *tile) {
  for_row_pieces<N, N / 16, G>(sl, [&](int r, int c16) {
    const u4 v = *reinterpret_cast<const u4 *>(src + (size_t)r * stride + 16 * c16);
    u4 lo, hi;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      lo[2 * k] = __builtin_amdgcn_perm(0u, v[k], 0x0c010c00u); lo[2 * k + 1] = __builtin_amdgcn_perm(0u, v[k], 0x0c030c02u);
      hi[2 * k] = __builtin_amdgcn_perm(0u, v[2 + k], 0x0c010c00u); hi[2 * k + 1] = __builtin_amdgcn_perm(0u, v[2 + k], 0x0c030c02u);
    }
    *reinterpret_cast<u4 *>(tile + r * N + 16 * c16) = lo;
    *reinterpret_cast<u4 *>(tile + r * N + 16 * c16 + 8) = hi;
  });
}
// 16-bit rows of N samples (16-byte aligned, stride ss) -> rows of stride ds, LDS to LDS or to HBM
template <int N, int G>
AV1MI_RP_FN void rows_copy(int sl, const uint16_t *src, int ss, uint16_t *dst, int ds) {
  for_row_pieces<N, N / 8, G>(sl, [&](int r, int c8) {
    *reinterpret_cast<u4 *>(dst + (size_t)r * ds + 8 * c8) = *reinterpret_cast<const u4 *>(src + r * ss + 8 * c8);
  });
}
// tile of N x N -> 16-bit rows in HBM
template <int N, int G>
AV1MI_RP_FN void tile_to_rows(int sl, const uint16_t *tile, uint16_t *dst, int stride) { rows_copy<N, G>(sl, tile, N, dst, stride); }
// ... -> 8-bit rows, narrowed: 16 samples per store
template <int N, int G>
AV1MI_RP_FN void tile_to_rows(int sl, const uint16_t *tile, uint8_t *dst, int stride) {
  for_row_pieces<N, N / 16, G>(sl, [&](int r, int c16) {
    const u4 lo = *reinterpret_cast<const u4 *>(tile + r * N + 16 * c16), hi = *reinterpret_cast<const u4 *>(tile + r * N + 16 * c16 + 8);
    u4 v;
    v[0] = __builtin_amdgcn_perm(lo[1], lo[0], 0x06040200u); v[1] = __builtin_amdgcn_perm(lo[3], lo[2], 0x06040200u);
    v[2] = __builtin_amdgcn_perm(hi[1], hi[0], 0x06040200u); v[3] = __builtin_amdgcn_perm(hi[3], hi[2], 0x06040200u);
    *reinterpret_cast<u4 *>(dst + (size_t)r * stride + 16 * c16) = v;
  });
}

// ---- the inverse networks pruned for a block's nonzero extent (txfm_gen.h): f(NzTag<inputs>) of the class nz, 64 = the full network.
// AV1MI_NO_PRUNE is the A/B switch: the build without the pruned networks.
template <int V> struct NzTag { static constexpr int value = V; };
#ifdef AV1MI_NO_PRUNE
constexpr bool PRUNE = false;
#else
constexpr bool PRUNE = true;
#endif
// the classes a size has pruned networks for
template <int LOG2N>
AV1MI_RP_FN int nz_class(int v) {
  if (!PRUNE) return 64;
  return LOG2N >= 5 ? (v <= 8 ? 8 : (v <= 16 ? 16 : 64)) : (LOG2N == 4 ? (v <= 4 ? 4 : (v <= 8 ? 8 : 64)) : (LOG2N == 3 && v <= 4 ? 4 : 64));
}
template <int LOG2N, typename F>
AV1MI_RP_FN void dispatch_nz(int nz, F f) {
  if constexpr (PRUNE) {
    if (LOG2N >= 4 && nz == 8) return f(NzTag<8>{});
    if (LOG2N >= 5 && nz == 16) return f(NzTag<16>{});
    if ((LOG2N == 3 || LOG2N == 4) && nz == 4) return f(NzTag<4>{});
  }
  f(NzTag<64>{});
}

}  // namespace av1mi_recon
#endif
