// fg_denoise_kernel.hip - the chunk's source denoised by its film-grain table before anything codes it (av1mi_params.film_grain bits 8 and
// 10; fg_denoise_rule.h is the rule).  One kernel on the main stream, behind fg_table_kernel, whose 24 values it
// reads where that kernel left them (Av1miFgBlock::table; launch_grain_passes runs the three film-grain passes in their order).  It works
// on tiles of the coded size, not on the estimate's 16x16 blocks: it shares nothing with the block walk of fg_rule.h and fg_pieces.h.
//
// Out of place: it reads the frames as the caller gave them - tight, at the signalled size - and writes the chunk's source at the coded
// size, so that chroma's index and every window see undenoised samples and the caller's memory is never written.  A workgroup takes a
// tile of 32 rows by 64 (16-bit samples) / 128 (8-bit samples) columns of one plane of one frame, of the CODED size: a lane of a row or
// column past the signalled picture computes the sample at the clamped position, which is the replication of the denoised edge
// (av1mi_launch_pad of the denoised frames) folded into the store.
//   stage    the tile with a halo of 2 samples, coordinates clamped to the signalled picture, as 16-bit samples in LDS; the plane's 256-entry
//            LUT in LDS; then T of every sample of the tile, one byte each, from the LUT at the sample's luma index - luma's own staged sample,
//            chroma's two luma samples read from the caller's frame
//   filter   a lane produces 16 bytes of horizontally adjacent outputs (8 / 16 samples) of one row: per window row it reads its outputs' samples and
//            the 4 beside them from LDS once and slides the five taps over them in registers; sums in 32 bits, one exact division per sample
//   store    16 bytes per lane (rows of the coded planes are 4-byte aligned); where the row ends inside the lane's samples, groups of four
// No table in scratch memory, no atomics; the staging loads are one sample per lane and coalesced - the filter's ~ 110 vector
// instructions per sample bound the kernel, not its loads.  Algorithmic HBM bytes per chunk: the caller's frames read once (plus the halo,
// 26 %, and for chroma the luma pairs, from the cache lines luma's tiles fetch), the coded frames written once.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "fg_denoise_rule.h"

namespace {

constexpr int FGD_THREADS = 256, FGD_LANES_X = 8, FGD_TH = FGD_THREADS / FGD_LANES_X, FGD_R = AV1MI_FGD_RADIUS;

// 16 bytes in one store to an address that is only known to be 4-byte aligned
typedef uint32_t FgdStore16 __attribute__((ext_vector_type(4), aligned(4)));

// n / d exactly, for n below 2^24 and d = 1 .. 1600 with a quotient up to 1 024 (av1mi_fgd_out's division): both convert to float exactly, the
// product with the reciprocal is within 2^-12 of n / d, so its floor is at most one off either way and the remainder corrects it - a
// quarter of the instructions of the 32-bit division
__device__ __forceinline__ uint32_t fgd_div(uint32_t n, uint32_t d) {
  uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d));
  const int r = (int)n - (int)(q * d);
  if (r < 0) q--;
  else if (r >= (int)d) q++;
  return q;
}

template <typename PIX>
__global__ void __launch_bounds__(FGD_THREADS) fg_denoise_kernel(Av1miDevParams P, const PIX *__restrict__ in, PIX *__restrict__ out,
                                                                 const uint8_t *__restrict__ table, int tiles_x_y, int tiles_y, int tiles_x_c, int tiles_c) {
  constexpr int NOUT = 16 / (int)sizeof(PIX), TW = FGD_LANES_X * NOUT, SW = TW + 2 * FGD_R, ROWS = FGD_TH + 2 * FGD_R, NW = (NOUT + 2 * FGD_R) / 2;
  constexpr int TS = SW + 2;   // samples per staged row (even: a lane's samples start on a word; 35 / 67 words: rows start on different banks)
  __shared__ __attribute__((aligned(16))) uint16_t tile[ROWS * TS];
  __shared__ __attribute__((aligned(16))) uint8_t reach[FGD_TH * TW];
  __shared__ uint8_t lut[256];
  const int t = threadIdx.x, f = blockIdx.y, bd = P.bit_depth;
  int b = blockIdx.x;
  const int plane = b < tiles_y ? 0 : (b < tiles_y + tiles_c ? 1 : 2);   // workgroup-uniform
  b -= plane == 0 ? 0 : (plane == 1 ? tiles_y : tiles_y + tiles_c);
  const int tiles_x = plane ? tiles_x_c : tiles_x_y;
  const int x0 = (b % tiles_x) * TW, y0 = (b / tiles_x) * FGD_TH;
  const int w = P.true_w, h = P.true_h, pw = plane ? w >> 1 : w, ph = plane ? h >> 1 : h;     // the signalled picture of the plane
  const int pcw = plane ? P.width >> 1 : P.width, pch = plane ? P.height >> 1 : P.height;     // ... and its coded size
  const size_t in_frame = (size_t)w * h * 3 / 2;
  const PIX *luma = in + (size_t)f * in_frame;
  const PIX *src = luma + (plane == 0 ? 0 : (plane == 1 ? (size_t)w * h : (size_t)w * h + (size_t)pw * ph));
  lut[t] = (uint8_t)av1mi_fgd_lut(table + plane * 8, t);
  for (int i = t; i < ROWS * SW; i += FGD_THREADS) {
    const int ly = i / SW, lx = i - ly * SW;
    int r = y0 - FGD_R + ly, c = x0 - FGD_R + lx;
    r = r < 0 ? 0 : (r < ph ? r : ph - 1); c = c < 0 ? 0 : (c < pw ? c : pw - 1);
    tile[ly * TS + lx] = (uint16_t)src[(size_t)r * pw + c];
  }
  __syncthreads();
  for (int i = t; i < FGD_TH * TW; i += FGD_THREADS) {
    const int ly = i / TW, lx = i - ly * TW;
    int index;
    if (plane == 0) {
      index = av1mi_fgd_index_luma((int)tile[(ly + FGD_R) * TS + lx + FGD_R], bd);
    } else {
      const int r = y0 + ly < ph ? y0 + ly : ph - 1, c = x0 + lx < pw ? x0 + lx : pw - 1;
      const PIX *q = luma + (size_t)(2 * r) * w + 2 * c;   // (w and h are even: 2 r < h and 2 c + 1 < w)
      index = av1mi_fgd_index_chroma((int)q[0], (int)q[1], bd);
    }
    reach[i] = (uint8_t)av1mi_fgd_reach((int)lut[index < 255 ? index : 255], bd);   // (a 16-bit sample above the format's maximum stays inside the LUT)
  }
  __syncthreads();
  // this lane's outputs: row y0 + ly of the coded plane, columns x .. x + NOUT - 1 (the first of them is inside the signalled picture:
  // the coded size is the signalled one rounded up to 8, x a multiple of 8)
  const int lx = t % FGD_LANES_X, ly = t / FGD_LANES_X, x = x0 + lx * NOUT;
  if (y0 + ly >= pch || x >= pcw) return;
  const int lr = (y0 + ly < ph ? y0 + ly : ph - 1) - y0;   // a row past the picture: the picture's last row (it is in this tile, likewise)
  int T[NOUT], xc[NOUT];
  uint32_t num[NOUT], den[NOUT];
  {
    const uint32_t *tw = reinterpret_cast<const uint32_t *>(reach + lr * TW + lx * NOUT);
#pragma unroll
    for (int j = 0; j < NOUT; j++) T[j] = (int)((tw[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    const uint32_t *cw = reinterpret_cast<const uint32_t *>(tile + (lr + FGD_R) * TS + lx * NOUT);
#pragma unroll
    for (int j = 0; j < NOUT; j++) { xc[j] = (int)((cw[(j + FGD_R) >> 1] >> (16 * ((j + FGD_R) & 1))) & 0xFFFFu); num[j] = 0; den[j] = 0; }
  }
#pragma unroll 1
  for (int dy = 0; dy < 2 * FGD_R + 1; dy++) {
    const uint32_t *rw = reinterpret_cast<const uint32_t *>(tile + (lr + dy) * TS + lx * NOUT);
    int s[2 * NW];
#pragma unroll
    for (int k = 0; k < NW; k++) { const uint32_t v = rw[k]; s[2 * k] = (int)(v & 0xFFFFu); s[2 * k + 1] = (int)(v >> 16); }
#pragma unroll
    for (int j = 0; j < NOUT; j++)
#pragma unroll
      for (int dx = 0; dx < 2 * FGD_R + 1; dx++) av1mi_fgd_tap(T[j], xc[j], s[j + dx], num[j], den[j]);
  }
  uint32_t o[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; j++) {
    o[j] = den[j] ? fgd_div(num[j] + den[j] / 2, den[j]) : (uint32_t)xc[j];   // av1mi_fgd_out
    if (j > 0 && x + j >= pw) o[j] = o[j - 1];   // a column past the picture: the denoised last column
  }
  uint32_t pk[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (sizeof(PIX) == 1) pk[k] = o[(4 * k) % NOUT] | (o[(4 * k + 1) % NOUT] << 8) | (o[(4 * k + 2) % NOUT] << 16) | (o[(4 * k + 3) % NOUT] << 24);
    else pk[k] = o[(2 * k) % NOUT] | (o[(2 * k + 1) % NOUT] << 16);   // (the modulo: the branch not taken still indexes inside o)
  }
  PIX *dst = out + (size_t)f * P.frame_samples + (plane == 0 ? 0 : (plane == 1 ? P.plane_off_u : P.plane_off_v)) + (size_t)(y0 + ly) * pcw + x;
  if (x + NOUT <= pcw) {
    const FgdStore16 v = { pk[0], pk[1], pk[2], pk[3] };
    *reinterpret_cast<FgdStore16 *>(dst) = v;
  } else {   // the row ends inside: whole groups of four samples (the coded planes' widths are multiples of 4)
    constexpr int WPG = 4 * (int)sizeof(PIX) / 4;   // words per group
    const int groups = (pcw - x) >> 2;
#pragma unroll
    for (int g = 0; g < NOUT / 4; g++)
      if (g < groups)
#pragma unroll
        for (int k = 0; k < WPG; k++) reinterpret_cast<uint32_t *>(dst)[g * WPG + k] = pk[g * WPG + k];
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_fg_denoise(const Av1miDevParams *P, const void *frames, void *out, const uint8_t *table, hipStream_t stream) {
  if (P->n_frames < 1 || ((uintptr_t)frames & 15) || ((uintptr_t)out & 15) || !table || frames == out) return hipErrorInvalidValue;
  if ((P->true_w & 1) || (P->true_h & 1) || P->true_w < 8 || P->true_h < 8 || P->width != ((P->true_w + 7) & ~7) || P->height != ((P->true_h + 7) & ~7) ||
      P->stride_y != P->width || P->stride_c != P->width / 2)
    return hipErrorInvalidValue;
  const int tw = FGD_LANES_X * (P->bit_depth == 8 ? 16 : 8);
  const int tx_y = (P->width + tw - 1) / tw, ty_y = (P->height + FGD_TH - 1) / FGD_TH;
  const int tx_c = (P->width / 2 + tw - 1) / tw, ty_c = (P->height / 2 + FGD_TH - 1) / FGD_TH;
  const dim3 grid((unsigned)(tx_y * ty_y + 2 * tx_c * ty_c), (unsigned)P->n_frames);
  if (P->bit_depth == 8)
    hipLaunchKernelGGL((fg_denoise_kernel<uint8_t>), grid, dim3(FGD_THREADS), 0, stream, *P, (const uint8_t *)frames, (uint8_t *)out, table, tx_y, tx_y * ty_y, tx_c, tx_c * ty_c);
  else
    hipLaunchKernelGGL((fg_denoise_kernel<uint16_t>), grid, dim3(FGD_THREADS), 0, stream, *P, (const uint16_t *)frames, (uint16_t *)out, table, tx_y, tx_y * ty_y, tx_c, tx_c * ty_c);
  return hipGetLastError();
}
