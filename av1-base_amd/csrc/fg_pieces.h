// fg_pieces.h - what the film-grain kernels share on the device.  fg_block_kernel (fg_kernel.hip) and fg_ar_sums_kernel (fg_ar_kernel.hip)
// stream the chunk's source along fg_rule.h's block walk: a lane's row by fg_row_at, its 16 samples in 16-byte loads, two 16-bit values per
// 32-bit lane exchange, the sum over a block's lanes.  fg_table_kernel and fg_ar_solve_kernel write a table's 24 header points (fg_put_points).
#ifndef AV1MI_FG_PIECES_H
#define AV1MI_FG_PIECES_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_dev.h"
#include "fg_rule.h"

// 16 / 8 bytes in one load from an address that is only known to be 4-byte aligned (8-bit chroma rows of a coded width that is not a
// multiple of 32)
struct __attribute__((aligned(4))) FgLoad16 { uint32_t w[4]; };
struct __attribute__((aligned(4))) FgLoad8 { uint32_t w[2]; };

// 16 samples from p into x; `full` = 0: only the first 8 exist, the rest read as 0
template <typename PIX>
__device__ __forceinline__ void fg_load_row(const PIX *p, bool full, int (&x)[16]) {
  if (sizeof(PIX) == 1) {
    uint32_t w[4] = { 0, 0, 0, 0 };
    if (full) { const FgLoad16 v = *reinterpret_cast<const FgLoad16 *>(p); w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3]; }
    else { const FgLoad8 v = *reinterpret_cast<const FgLoad8 *>(p); w[0] = v.w[0]; w[1] = v.w[1]; }
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
  } else {
    uint32_t w[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    { const FgLoad16 v = *reinterpret_cast<const FgLoad16 *>(p); w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3]; }
    if (full) { const FgLoad16 v = *reinterpret_cast<const FgLoad16 *>(p + 8); w[4] = v.w[0]; w[5] = v.w[1]; w[6] = v.w[2]; w[7] = v.w[3]; }
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = (int)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
  }
}

// where a walk's lane (fg_rule.h) reads: row `row` of block (by, bx) of frame f in the frames at the coded size - 16 luma samples, or in
// plane 1 / 2 the 8 U / V samples of that block with the right neighbour's 8 behind them
template <typename PIX>
__device__ __forceinline__ const PIX *fg_row_at(const Av1miDevParams &P, const PIX *frames, int plane, int f, int by, int bx, int row) {
  const PIX *fr = frames + (size_t)f * P.frame_samples;
  if (plane == 0) return fr + (size_t)(by * 16 + row) * P.stride_y + bx * 16;
  return fr + (plane == 1 ? P.plane_off_u : P.plane_off_v) + (size_t)(by * 8 + row) * P.stride_c + bx * 8;
}

// two values of 16 bits in the one word a lane exchange moves
__device__ __forceinline__ uint32_t fg_pack2(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int fg_lo16(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
__device__ __forceinline__ int fg_hi16(uint32_t v) { return (int)v >> 16; }

// v summed over the `lanes` (a power of two) consecutive lanes this one is among, in every one of them; every lane of the wave comes here
template <class T>
__device__ __forceinline__ T fg_sum_lanes(T v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the table v[plane][bin] into the frame header at h, whose first luma point value stands at bit offset `bit` + 8 (fg_rule.h: the points)
__device__ __forceinline__ void fg_put_points(uint8_t *h, int bit, const int *v) {
  for (int pl = 0; pl < 3; pl++)
    for (int k = 0; k < AV1MI_FG_BINS; k++)
      av1mi_fg_put8(h, bit + (pl == 0 ? 0 : (pl == 1 ? AV1MI_FG_CB_BIT : AV1MI_FG_CR_BIT)) + 16 * k + 8, (uint32_t)v[pl * AV1MI_FG_BINS + k]);
}

#endif
