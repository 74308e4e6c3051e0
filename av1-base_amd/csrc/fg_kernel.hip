// fg_kernel.hip - the film-grain table estimated from a chunk's source (av1mi_params.film_grain bit 8; fg_rule.h is
// the rule).  Two kernels on the main stream, before anything else reads or patches the chunk:
//
// fg_block_kernel: a streaming pass over Y, U and V that reads every sample of a counted block from HBM once, 16 bytes per load.  A lane
// holds 16 consecutive samples of one row: a luma block's row, or the U (V) row of a PAIR of horizontally adjacent blocks - 2 x 8 samples,
// so chroma rows load as wide as luma rows.  The horizontal second difference is formed in the lane, the vertical one from the lanes above
// and below it (rows of a block sit in consecutive lanes; two 16-bit differences per 32-bit exchange), then |.| summed over the interior
// columns and rows and reduced over the block's 16 (8) lanes.  A workgroup of three waves takes four pairs at a time: waves 0 and 1 their
// eight luma blocks, wave 2 the four U and four V pair-rows, so no wave diverges; the eight records { bin, v_y, v_u, v_v } meet in LDS and
// go out as one 4-byte store per block.  No atomics.  Algorithmic HBM bytes per chunk of n frames: n L b 3 / 2 read (L luma samples of
// the counted blocks, b bytes each), 4 n L / 256 written.
// fg_hist_kernel: the 3 x 8 histograms of 256 counters from those records, in up to 64 parts: a workgroup tallies its slice of the records
// in LDS (integer counts: exact, any order gives the same) and stores its part - store and sum, no global atomics.  (One workgroup for
// all records was measured first: on content whose blocks share few values the adds queue up at a few LDS counters, 0.45 ms of a
// 1080p x 60 chunk's 0.58.)
// fg_table_kernel: one workgroup.  The parts' sum into LDS, the quartiles, the fill and the clamp; the table and the counts to memory, and
// the 24 values into every frame's header slot at fg_bit, one lane per header; the quartiles before fill and clamp for fg_ar_kernel.hip.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "fg_rule.h"
#include "fg_pieces.h"

namespace {

// sum |M * x| of this lane's row over the columns 1 .. 6, 7 .. 8 and 9 .. 14 (zeros unless `interior`: the row has both neighbours inside its
// block, which are the lanes before and after this one)
__device__ __forceinline__ void fg_row_response(const int (&x)[16], bool interior, uint32_t &left, uint32_t &mid, uint32_t &right) {
  int h[14];
#pragma unroll
  for (int c = 0; c < 14; c++) h[c] = x[c] - 2 * x[c + 1] + x[c + 2];   // (|h| <= 4 * 1023: 16 bits hold it)
  uint32_t s[3] = { 0, 0, 0 };
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const uint32_t pk = ((uint32_t)h[2 * j] & 0xFFFFu) | ((uint32_t)h[2 * j + 1] << 16);
    const uint32_t up = __shfl_up(pk, 1, 64), dn = __shfl_down(pk, 1, 64);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int a = k ? (int)up >> 16 : (int)(int16_t)(up & 0xFFFFu), d = k ? (int)dn >> 16 : (int)(int16_t)(dn & 0xFFFFu);
      const int r = a - 2 * h[2 * j + k] + d, c = 2 * j + k;   // column c + 1
      s[c < 6 ? 0 : (c < 8 ? 1 : 2)] += (uint32_t)(r < 0 ? -r : r);
    }
  }
  left = interior ? s[0] : 0; mid = interior ? s[1] : 0; right = interior ? s[2] : 0;
}

constexpr int FG_THREADS = 192, FG_SLOTS = 8;   // block slots of a workgroup's step: four pairs

template <typename PIX>
__global__ void __launch_bounds__(FG_THREADS) fg_block_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ blocks) {
  __shared__ uint32_t rec[FG_SLOTS];
  const int nbx = av1mi_fg_blocks(P.true_w), nby = av1mi_fg_blocks(P.true_h), npx = (nbx + 1) / 2;
  const long n_pairs = (long)P.n_frames * nby * npx, n_steps = (n_pairs + 3) / 4;
  const int t = threadIdx.x;
  const bool luma = t < 128;   // wave-uniform
  // this lane's slot, plane and row
  const int slot = luma ? t >> 4 : ((t >> 3) & 3) * 2, row = luma ? t & 15 : t & 7, plane = luma ? 0 : 1 + ((t - 128) >> 5);
  for (long step = blockIdx.x; step < n_steps; step += gridDim.x) {
    // block of a slot: pair (step * 4 + slot / 2), side slot & 1
    auto locate = [&](int sl, int &f, int &by, int &bx) {
      const long gp = step * 4 + (sl >> 1);
      f = (int)(gp / ((long)nby * npx));
      const int in = (int)(gp % ((long)nby * npx));
      by = in / npx; bx = (in % npx) * 2 + (sl & 1);
      return gp < n_pairs && bx < nbx;
    };
    int f, by, bx;
    const bool here = locate(slot, f, by, bx);
    if (luma) {
      uint32_t S = 0, N = 0;
      if (here) {   // (uniform over the block's 16 lanes: the exchanges below stay inside them)
        int x[16];
        fg_load_row<PIX>(frames + (size_t)f * P.frame_samples + (size_t)(by * 16 + row) * P.stride_y + bx * 16, true, x);
#pragma unroll
        for (int i = 0; i < 16; i++) S += (uint32_t)x[i];
        uint32_t l, m, r;
        fg_row_response(x, row > 0 && row < 15, l, m, r);
        N = l + m + r;
      }
      for (int o = 8; o > 0; o >>= 1) { S += __shfl_xor(S, o, 64); N += __shfl_xor(N, o, 64); }
      if (row == 0) rec[slot] = (uint32_t)av1mi_fg_bin(S, P.bit_depth) | ((uint32_t)av1mi_fg_value(N, 0, P.bit_depth) << 8);
    }
    __syncthreads();   // (the luma lanes store whole records, the chroma lanes then their bytes)
    if (!luma) {
      uint32_t l = 0, m, r = 0;
      if (here) {   // the pair's left block exists; its right block may not
        int x[16];
        const bool both = bx + 1 < nbx;
        fg_load_row<PIX>(frames + (size_t)f * P.frame_samples + (plane == 1 ? P.plane_off_u : P.plane_off_v) + (size_t)(by * 8 + row) * P.stride_c + bx * 8, both, x);
        fg_row_response(x, row > 0 && row < 7, l, m, r);
      }
      for (int o = 4; o > 0; o >>= 1) { l += __shfl_xor(l, o, 64); r += __shfl_xor(r, o, 64); }
      if (row == 0) {
        reinterpret_cast<uint8_t *>(rec)[slot * 4 + 1 + plane] = (uint8_t)av1mi_fg_value(l, 1, P.bit_depth);
        reinterpret_cast<uint8_t *>(rec)[(slot + 1) * 4 + 1 + plane] = (uint8_t)av1mi_fg_value(r, 1, P.bit_depth);
      }
    }
    __syncthreads();
    if (t < FG_SLOTS && locate(t, f, by, bx)) blocks[((size_t)f * nby + by) * nbx + bx] = rec[t];
    __syncthreads();   // (the next step's records)
  }
}

constexpr int FG_TABLE_THREADS = 1024, FG_HIST_STRIDE = 257;   // (the stride: the 24 lanes that scan the histograms start on 24 banks)
constexpr int FG_HIST_WORDS = AV1MI_FG_TABLE * 256;            // counters of one part
constexpr size_t FG_PART_RECORDS = 8192;                       // records a part holds at least, while there are parts left

// part blockIdx.x of the 3 x 8 histograms: the records [part * per, (part + 1) * per) tallied in LDS, then stored (per: a multiple of 4)
__global__ void __launch_bounds__(FG_TABLE_THREADS) fg_hist_kernel(const uint32_t *__restrict__ blocks, size_t n, size_t per, uint32_t *__restrict__ parts) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[FG_HIST_WORDS];
  const int t = threadIdx.x;
  for (int i = t; i < FG_HIST_WORDS; i += FG_TABLE_THREADS) hist[i] = 0;
  __syncthreads();
  auto tally = [&](uint32_t r) {
    const uint32_t bin = r & 7u;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) atomicAdd(&hist[(pl * AV1MI_FG_BINS + bin) * 256 + ((r >> (8 + 8 * pl)) & 0xFFu)], 1u);
  };
  const size_t from = (size_t)blockIdx.x * per, to = from + per < n ? from + per : n;   // (from < n: the launcher's part count)
  const size_t q0 = from / 4, q1 = to / 4;   // (the records are 16-byte aligned, `from` is a multiple of 4)
  for (size_t i = q0 + t; i < q1; i += FG_TABLE_THREADS) {
    const uint4 r = reinterpret_cast<const uint4 *>(blocks)[i];
    tally(r.x); tally(r.y); tally(r.z); tally(r.w);
  }
  for (size_t i = q1 * 4 + t; i < to; i += FG_TABLE_THREADS) tally(blocks[i]);
  __syncthreads();
  uint4 *out = reinterpret_cast<uint4 *>(parts + (size_t)blockIdx.x * FG_HIST_WORDS);
  for (int i = t; i < FG_HIST_WORDS / 4; i += FG_TABLE_THREADS) out[i] = reinterpret_cast<const uint4 *>(hist)[i];
}

__global__ void __launch_bounds__(FG_TABLE_THREADS) fg_table_kernel(Av1miDevParams P, const uint32_t *__restrict__ parts, int n_parts, int ceil_y, int ceil_c,
                                                                    uint8_t *__restrict__ table, uint32_t *__restrict__ counts, uint8_t *__restrict__ quart, uint8_t *__restrict__ hdr_blob,
                                                                    int bit_key, int bit_inter) {
  __shared__ uint32_t hist[AV1MI_FG_TABLE * FG_HIST_STRIDE];
  __shared__ uint32_t count[AV1MI_FG_TABLE];
  __shared__ int value[AV1MI_FG_TABLE], final_v[AV1MI_FG_TABLE];
  const int t = threadIdx.x;
  for (int e = t; e < FG_HIST_WORDS; e += FG_TABLE_THREADS) {   // the parts' sum, counter by counter
    uint32_t c = 0;
    for (int g = 0; g < n_parts; g++) c += parts[(size_t)g * FG_HIST_WORDS + e];
    hist[(e >> 8) * FG_HIST_STRIDE + (e & 255)] = c;
  }
  __syncthreads();
  if (t < AV1MI_FG_TABLE) {
    const uint32_t *h = hist + t * FG_HIST_STRIDE;
    uint32_t c = 0;
    for (int v = 0; v < 256; v++) c += h[v];
    count[t] = c;
    value[t] = c ? av1mi_fg_quartile(h, c) : 0;
  }
  __syncthreads();
  if (t < AV1MI_FG_TABLE) {
    const int pl = t / AV1MI_FG_BINS;
    const int v = av1mi_fg_fill(count + pl * AV1MI_FG_BINS, value + pl * AV1MI_FG_BINS, t % AV1MI_FG_BINS, pl ? ceil_c : ceil_y);
    final_v[t] = v;
    table[t] = (uint8_t)v;
    counts[t] = count[t];
    if (quart) quart[t] = (uint8_t)value[t];   // before the fill and the ceiling: what fg_ar_kernel.hip calls a block flat by
  }
  __syncthreads();
  if (!hdr_blob) return;
  for (int f = t; f < P.n_frames; f += FG_TABLE_THREADS) {   // one writer per header
    uint8_t *h = hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
    const int bit = av1mi_frame_is_inter(P, f) ? bit_inter : bit_key;
    for (int pl = 0; pl < 3; pl++)
      for (int k = 0; k < AV1MI_FG_BINS; k++)
        av1mi_fg_put8(h, bit + (pl == 0 ? 0 : (pl == 1 ? AV1MI_FG_CB_BIT : AV1MI_FG_CR_BIT)) + 16 * k + 8, (uint32_t)final_v[pl * AV1MI_FG_BINS + k]);
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_film_grain(const Av1miDevParams *P, const void *frames, uint32_t *blocks, uint32_t *parts, uint8_t *table, uint32_t *counts,
                                              uint8_t *quart, int ceil_y, int ceil_c, uint8_t *hdr_blob, int bit_key, int bit_inter, hipStream_t stream) {
  if (P->n_frames < 1 || ((uintptr_t)frames & 15) || ((uintptr_t)blocks & 15) || ((uintptr_t)parts & 15) || (hdr_blob && (bit_key <= 0 || bit_inter <= 0))) return hipErrorInvalidValue;
  const int nbx = av1mi_fg_blocks(P->true_w), nby = av1mi_fg_blocks(P->true_h);
  const size_t n = (size_t)P->n_frames * nbx * nby;
  if (n) {   // (a picture smaller than a block has none: the table is all 0)
    const long n_steps = ((long)P->n_frames * nby * ((nbx + 1) / 2) + 3) / 4;
    const dim3 grid((unsigned)(n_steps < 4096 ? n_steps : 4096));
    if (P->bit_depth == 8) hipLaunchKernelGGL((fg_block_kernel<uint8_t>), grid, dim3(FG_THREADS), 0, stream, *P, (const uint8_t *)frames, blocks);
    else hipLaunchKernelGGL((fg_block_kernel<uint16_t>), grid, dim3(FG_THREADS), 0, stream, *P, (const uint16_t *)frames, blocks);
  }
  // the histograms in parts of at least FG_PART_RECORDS records, at most AV1MI_FG_PARTS of them; every part's slice starts on a 16-byte boundary
  size_t n_parts = (n + FG_PART_RECORDS - 1) / FG_PART_RECORDS;
  if (n_parts > AV1MI_FG_PARTS) n_parts = AV1MI_FG_PARTS;
  if (n_parts) {
    const size_t per = ((n + n_parts - 1) / n_parts + 3) & ~(size_t)3;
    n_parts = (n + per - 1) / per;
    hipLaunchKernelGGL(fg_hist_kernel, dim3((unsigned)n_parts), dim3(FG_TABLE_THREADS), 0, stream, (const uint32_t *)blocks, n, per, parts);
  }
  hipLaunchKernelGGL(fg_table_kernel, dim3(1), dim3(FG_TABLE_THREADS), 0, stream, *P, (const uint32_t *)parts, (int)n_parts, ceil_y, ceil_c, table, counts,
                     quart, hdr_blob, bit_key, bit_inter);
  return hipGetLastError();
}
