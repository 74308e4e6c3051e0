// fg_pieces.h - what the film-grain kernels that stream the chunk's source share (fg_kernel.hip, fg_ar_kernel.hip): a lane's row of 16
// samples in 16-byte loads.
#ifndef AV1MI_FG_PIECES_H
#define AV1MI_FG_PIECES_H
#include <hip/hip_runtime.h>
#include <stdint.h>

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

#endif
