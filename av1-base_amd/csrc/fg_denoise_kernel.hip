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
//
// The temporal term (bits 14 and 15 of the field) is a template parameter of the filter kernel - without it the
// kernel is the one above - and a search launch in front of it.  fgd_search_kernel: per (16x16 block, slot, frame) one wave runs
// tf_search.h's full search of frame f in its neighbour g on the undenoised frames at the coded size, one 32-bit key each (fg_denoise_rule.h
// has the layout).  The filter kernel then takes the neighbours one after the other through one LDS buffer: per 16x16 luma / 8x8 chroma
// block of the tile the block's vector, then the (16 + 2)^2 / (8 + 2)^2 patch of the neighbour's plane the block's 3x3 windows lie in, every
// coordinate clamped by itself, a barrier, the lanes' taps from the patch into the sums they hold in registers, a barrier.  13 KB of LDS
// at most beside the tile, whatever the span.  Added HBM bytes per chunk: the luma planes read (1 + 2 S)-fold by the search (the
// candidates' re-reads are cache hits), the neighbours' patches - 1.27 (luma) / 1.56 (chroma) times the frame per neighbour - and the keys.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "fg_denoise_rule.h"
#include "tf_search.h"

namespace {

constexpr int FGD_THREADS = 256, FGD_LANES_X = 8, FGD_TH = FGD_THREADS / FGD_LANES_X, FGD_R = AV1MI_FGD_RADIUS;

// 16 bytes in one store to an address that is only known to be 4-byte aligned
typedef uint32_t FgdStore16 __attribute__((ext_vector_type(4), aligned(4)));

// n / d exactly, for n below 2^24 and d = 1 .. 4672 with a quotient up to 1 024 (av1mi_fgd_out's division; 1600 is the spatial filter's
// largest d, 4672 = 1600 + 4 * 12 * 64 the largest with four neighbours, where n = num + d / 2 <= 4672 * 1023 + 2336 < 2^23): both convert to
// float exactly whatever d below 2^24 is, the reciprocal is within one unit in the last place of 1 / d and the product rounds once more,
// a relative error below 2^-22 that does not depend on d, so at a quotient up to 2^10 the product is within 2^-12 of n / d, its floor
// is at most one off either way and the remainder corrects it - a quarter of the instructions of the 32-bit division
__device__ __forceinline__ uint32_t fgd_div(uint32_t n, uint32_t d) {
  uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d));
  const int r = (int)n - (int)(q * d);
  if (r < 0) q--;
  else if (r >= (int)d) q++;
  return q;
}

// ---- the temporal term's pieces
constexpr int FGD_NO_VECTOR = 0x7FFF0000;   // a block without this neighbour; else (dy << 16) | (dx & 0xFFFF) of the plane

// the search: the key of (frame f, slot, block b), all-ones where frame f has no such neighbour within the span
template <typename PIX, int R>
__global__ void __launch_bounds__(64) fgd_search_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ mv, int span) {
  const int W = P.width, H = P.height, nbx = av1mi_tf_blocks(W), nb = nbx * av1mi_tf_blocks(H);
  const int b = blockIdx.x, slot = blockIdx.y, f = blockIdx.z, lane = threadIdx.x;
  uint32_t *dst = mv + ((size_t)f * AV1MI_FGD_SLOTS + slot) * nb + b;
  if (!av1mi_fgd_slot_exists(f, slot, span, P.n_frames)) {
    if (lane == 0) *dst = AV1MI_FGD_NONE;
    return;
  }
  const PIX *cur = frames + (size_t)f * P.frame_samples, *ref = frames + (size_t)(f + av1mi_fgd_slot_offset(slot)) * P.frame_samples;
  // (`frames` is 16-byte aligned, and the rows' strides and the frames' sizes are multiples of 8: tf_search.h loads whole words)
  uint32_t s2[8];
  const uint32_t best = tf_search_block<PIX, R>(cur, ref, (b % nbx) * AV1MI_TF_BLOCK, (b / nbx) * AV1MI_TF_BLOCK, W, H, P.stride_y, lane, s2);
  if (lane == 0) *dst = best;
}

// the patches of one neighbour's plane `nsrc` (pw x ph, the signalled picture) for the tile at (x0, y0): per block k of B x B samples with a
// vector the (B + 2)^2 samples its windows lie in, each coordinate clamped by itself
template <typename PIX, int B, int TW>
__device__ __forceinline__ void fgd_stage_patches(uint16_t *patch, const int *vec, const PIX *__restrict__ nsrc, int pw, int ph, int x0, int y0, int t) {
  constexpr int PW = B + 2, PS = PW * PW, TBX = TW / B, NTB = TBX * (FGD_TH / B);
  for (int i = t; i < NTB * PS; i += FGD_THREADS) {
    const int k = i / PS, o = i - k * PS, py = o / PW, px = o - py * PW, v = vec[k];
    if (v == FGD_NO_VECTOR) continue;
    const int ky = k / TBX, kx = k - ky * TBX;
    int r = y0 + ky * B + py - 1 + (v >> 16), c = x0 + kx * B + px - 1 + (int)(int16_t)(v & 0xFFFF);
    r = r < 0 ? 0 : (r < ph ? r : ph - 1); c = c < 0 ? 0 : (c < pw ? c : pw - 1);
    patch[i] = (uint16_t)nsrc[(size_t)r * pw + c];
  }
}
// ... and a lane's taps from them: its NOUT outputs of tile row lr from tile column lx * NOUT on, eight at a time (eight lie in one block)
template <int B, int TW, int NOUT>
__device__ __forceinline__ void fgd_window_taps(const uint16_t *patch, const int *vec, int lr, int lx, const int (&T)[NOUT], const int (&xc)[NOUT],
                                                uint32_t (&num)[NOUT], uint32_t (&den)[NOUT]) {
  constexpr int PW = B + 2, PS = PW * PW, TBX = TW / B;
  const int ky = lr / B, iy = lr - ky * B;
#pragma unroll
  for (int q = 0; q < NOUT / 8; q++) {
    const int cx = lx * NOUT + 8 * q, kx = cx / B, ix = cx - kx * B, k = ky * TBX + kx;
    if (vec[k] == FGD_NO_VECTOR) continue;
    const uint16_t *p = patch + k * PS + iy * PW + ix;   // rows iy .. iy + 2 and columns ix .. ix + 9 of the patch: the eight samples' windows
#pragma unroll
    for (int ty = 0; ty < 3; ty++) {
      int s[10];
#pragma unroll
      for (int i = 0; i < 10; i++) s[i] = (int)p[ty * PW + i];
#pragma unroll
      for (int j = 0; j < 8; j++)
#pragma unroll
        for (int tx = 0; tx < 3; tx++)
          av1mi_fgd_tap_times(ty == 1 && tx == 1 ? AV1MI_FGD_CENTRE_WEIGHT : 1, T[8 * q + j], xc[8 * q + j], s[j + tx], num[8 * q + j], den[8 * q + j]);
    }
  }
}

// TEMPORAL: the neighbours' windows on top (mv: the search's keys, span: 1 or 2); without it mv and span are not looked at
template <typename PIX, bool TEMPORAL>
__global__ void __launch_bounds__(FGD_THREADS) fg_denoise_kernel(Av1miDevParams P, const PIX *__restrict__ in, PIX *__restrict__ out,
                                                                 const uint8_t *__restrict__ table, int tiles_x_y, int tiles_y, int tiles_x_c, int tiles_c,
                                                                 const uint32_t *__restrict__ mv, int span) {
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
  const bool idle = y0 + ly >= pch || x >= pcw;   // nothing to store
  if constexpr (!TEMPORAL) {
    if (idle) return;
  }   // (with the temporal term the lane stays for the barriers: what it computes lies inside the tile, and it stores nothing)
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
  if constexpr (TEMPORAL) {
    constexpr int MAXB = (FGD_TH / 8) * (TW / 8);   // the chroma blocks of a tile, four times its luma blocks
    __shared__ uint16_t patch[MAXB * 100];          // chroma: 10 x 10 per block; luma: 18 x 18 per four of them
    __shared__ int vec[MAXB];
    const int R = P.me_range, nbx = av1mi_tf_blocks(P.width), nby = av1mi_tf_blocks(P.height), bl2 = plane ? 3 : 4;
    const int tbx = TW >> bl2, ntb = tbx * (FGD_TH >> bl2);
#pragma unroll 1
    for (int slot = 0; slot < AV1MI_FGD_SLOTS; slot++) {
      if (!av1mi_fgd_slot_exists(f, slot, span, P.n_frames)) continue;   // (workgroup-uniform)
      const PIX *nsrc = src + (ptrdiff_t)av1mi_fgd_slot_offset(slot) * (ptrdiff_t)in_frame;
      if (t < ntb) {   // the tile's blocks' vectors; a block past the grid takes the last one's (nothing of it is stored)
        const int ky = t / tbx, kx = t - ky * tbx;
        const int by = (y0 >> bl2) + ky < nby ? (y0 >> bl2) + ky : nby - 1, bx = (x0 >> bl2) + kx < nbx ? (x0 >> bl2) + kx : nbx - 1;
        const uint32_t key = mv[((size_t)f * AV1MI_FGD_SLOTS + slot) * ((size_t)nbx * nby) + (size_t)by * nbx + bx];
        int v = FGD_NO_VECTOR;
        if (key != AV1MI_FGD_NONE) {
          int dy, dx;
          av1mi_fgd_vector(key, R, &dy, &dx);
          if (plane) { dy = av1mi_fgd_chroma_shift(dy); dx = av1mi_fgd_chroma_shift(dx); }
          v = dy * 65536 + (dx & 0xFFFF);
        }
        vec[t] = v;
      }
      __syncthreads();
      if (plane == 0) fgd_stage_patches<PIX, 16, TW>(patch, vec, nsrc, pw, ph, x0, y0, t);
      else fgd_stage_patches<PIX, 8, TW>(patch, vec, nsrc, pw, ph, x0, y0, t);
      __syncthreads();
      if (plane == 0) fgd_window_taps<16, TW, NOUT>(patch, vec, lr, lx, T, xc, num, den);
      else fgd_window_taps<8, TW, NOUT>(patch, vec, lr, lx, T, xc, num, den);
      __syncthreads();   // the next neighbour overwrites the vectors and the patches
    }
    if (idle) return;
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

extern "C" hipError_t av1mi_launch_fg_denoise_search(const Av1miDevParams *P, const void *coded, uint32_t *mv, int span, hipStream_t stream) {
  if (span < 1 || span > 2 || (P->me_range != 8 && P->me_range != 16) || P->n_frames < 1 || !mv || ((uintptr_t)coded & 15) || (P->width & 7) || (P->height & 7) ||
      P->stride_y != P->width)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(av1mi_tf_blocks(P->width) * av1mi_tf_blocks(P->height)), AV1MI_FGD_SLOTS, (unsigned)P->n_frames);
  if (P->bit_depth == 8) {
    if (P->me_range == 16) hipLaunchKernelGGL((fgd_search_kernel<uint8_t, 16>), grid, dim3(64), 0, stream, *P, (const uint8_t *)coded, mv, span);
    else hipLaunchKernelGGL((fgd_search_kernel<uint8_t, 8>), grid, dim3(64), 0, stream, *P, (const uint8_t *)coded, mv, span);
  } else {
    if (P->me_range == 16) hipLaunchKernelGGL((fgd_search_kernel<uint16_t, 16>), grid, dim3(64), 0, stream, *P, (const uint16_t *)coded, mv, span);
    else hipLaunchKernelGGL((fgd_search_kernel<uint16_t, 8>), grid, dim3(64), 0, stream, *P, (const uint16_t *)coded, mv, span);
  }
  return hipGetLastError();
}

template <typename PIX>
static void fgd_launch(const Av1miDevParams *P, const void *frames, void *out, const uint8_t *table, const uint32_t *mv, int span, dim3 grid, int tx_y, int ty_y,
                       int tx_c, int ty_c, hipStream_t stream) {
  if (span)
    hipLaunchKernelGGL((fg_denoise_kernel<PIX, true>), grid, dim3(FGD_THREADS), 0, stream, *P, (const PIX *)frames, (PIX *)out, table, tx_y, tx_y * ty_y, tx_c, tx_c * ty_c, mv, span);
  else
    hipLaunchKernelGGL((fg_denoise_kernel<PIX, false>), grid, dim3(FGD_THREADS), 0, stream, *P, (const PIX *)frames, (PIX *)out, table, tx_y, tx_y * ty_y, tx_c, tx_c * ty_c, mv, span);
}

extern "C" hipError_t av1mi_launch_fg_denoise(const Av1miDevParams *P, const void *frames, void *out, const uint8_t *table, const uint32_t *mv, int span,
                                              hipStream_t stream) {
  if (P->n_frames < 1 || ((uintptr_t)frames & 15) || ((uintptr_t)out & 15) || !table || frames == out) return hipErrorInvalidValue;
  if (span < 0 || span > 2 || (span && (!mv || (P->me_range != 8 && P->me_range != 16)))) return hipErrorInvalidValue;
  if ((P->true_w & 1) || (P->true_h & 1) || P->true_w < 8 || P->true_h < 8 || P->width != ((P->true_w + 7) & ~7) || P->height != ((P->true_h + 7) & ~7) ||
      P->stride_y != P->width || P->stride_c != P->width / 2)
    return hipErrorInvalidValue;
  const int tw = FGD_LANES_X * (P->bit_depth == 8 ? 16 : 8);
  const int tx_y = (P->width + tw - 1) / tw, ty_y = (P->height + FGD_TH - 1) / FGD_TH;
  const int tx_c = (P->width / 2 + tw - 1) / tw, ty_c = (P->height / 2 + FGD_TH - 1) / FGD_TH;
  const dim3 grid((unsigned)(tx_y * ty_y + 2 * tx_c * ty_c), (unsigned)P->n_frames);
  if (P->bit_depth == 8) fgd_launch<uint8_t>(P, frames, out, table, mv, span, grid, tx_y, ty_y, tx_c, ty_c, stream);
  else fgd_launch<uint16_t>(P, frames, out, table, mv, span, grid, tx_y, ty_y, tx_c, ty_c, stream);
  return hipGetLastError();
}
