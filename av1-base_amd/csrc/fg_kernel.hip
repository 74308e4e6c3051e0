// fg_kernel.hip - the film-grain table estimated from a chunk's source (av1mi_params.film_grain bit 8; fg_rule.h is
// the rule).  Two kernels on the main stream, before anything else reads or patches the chunk:
//
// fg_block_kernel: a streaming pass over Y, U and V that reads every sample of a counted block from HBM once, 16 bytes per load.  A lane
// holds 16 consecutive samples of one row: a luma block's row, or the U (V) row of a PAIR of horizontally adjacent blocks - 2 x 8 samples,
// so chroma rows load as wide as luma rows.  The horizontal second difference is formed in the lane, the vertical one from the lanes above
// and below it (rows of a block sit in consecutive lanes; two 16-bit differences per 32-bit exchange), then |.| summed over the interior
// columns and rows and reduced over the block's 16 (8) lanes.  Lanes and blocks are placed by fg_rule.h's block walk, which
// fg_ar_sums_kernel shares (the row's address, load, packing and lane sums: fg_pieces.h): a workgroup of three waves takes four pairs at
// a time, waves 0 and 1 their eight luma blocks, wave 2 the four U and four V pair-rows, so no wave diverges; the eight records
// { bin, v_y, v_u, v_v } meet in LDS and go out as one 4-byte store per block.  No atomics.  Algorithmic HBM bytes per chunk of n frames:
// n L b 3 / 2 read (L luma samples of the counted blocks, b bytes each), 4 n L / 256 written.
// fg_hist_kernel: the 3 x 8 histograms of 256 counters from those records, in up to 64 parts: a workgroup tallies its slice of the records
// in LDS (integer counts: exact, any order gives the same) and stores its part - store and sum, no global atomics.  (One workgroup for
// all records was measured first: on content whose blocks share few values the adds queue up at a few LDS counters, 0.45 ms of a
// 1080p x 60 chunk's 0.58.)
// fg_table_kernel: one workgroup.  The parts' sum into LDS, the quartiles, the fill and the clamp; the table and the counts to memory, and
// the 24 values into every frame's header slot at fg_bit, one lane per header (fg_pieces.h's writer, which fg_ar_solve_kernel uses over
// them); the quartiles before fill and clamp for fg_ar_kernel.hip.
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
    const uint32_t pk = fg_pack2(h[2 * j], h[2 * j + 1]);
    const uint32_t up = __shfl_up(pk, 1, 64), dn = __shfl_down(pk, 1, 64);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int a = k ? fg_hi16(up) : fg_lo16(up), d = k ? fg_hi16(dn) : fg_lo16(dn);
      const int r = a - 2 * h[2 * j + k] + d, c = 2 * j + k;   // column c + 1
      s[c < 6 ? 0 : (c < 8 ? 1 : 2)] += (uint32_t)(r < 0 ? -r : r);
    }
  }
  left = interior ? s[0] : 0; mid = interior ? s[1] : 0; right = interior ? s[2] : 0;
}

template <typename PIX>
__global__ void __launch_bounds__(AV1MI_FG_WALK_THREADS) fg_block_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ blocks) {
  __shared__ uint32_t rec[AV1MI_FG_WALK_SLOTS];
  const int nbx = av1mi_fg_blocks(P.true_w), nby = av1mi_fg_blocks(P.true_h), t = threadIdx.x;
  const long n_steps = av1mi_fg_walk_steps(P.n_frames, nbx, nby);
  const Av1miFgLane L = av1mi_fg_walk_lane(t);
  // (every thread of the workgroup takes the same steps: the three barriers of a step are reached by all of them)
  for (long step = blockIdx.x; step < n_steps; step += gridDim.x) {
    const Av1miFgSpot b = av1mi_fg_walk_spot(step, L.slot, P.n_frames, nbx, nby);
    if (L.luma) {
      uint32_t S = 0, N = 0;
      if (b.here) {   // (uniform over the block's 16 lanes: the exchanges below stay inside them)
        int x[16];
        fg_load_row<PIX>(fg_row_at(P, frames, 0, b.f, b.by, b.bx, L.row), true, x);
#pragma unroll
        for (int i = 0; i < 16; i++) S += (uint32_t)x[i];
        uint32_t l, m, r;
        fg_row_response(x, L.row > 0 && L.row < 15, l, m, r);
        N = l + m + r;
      }
      S = fg_sum_lanes(S, 16); N = fg_sum_lanes(N, 16);
      if (L.row == 0) rec[L.slot] = (uint32_t)av1mi_fg_bin(S, P.bit_depth) | ((uint32_t)av1mi_fg_value(N, 0, P.bit_depth) << 8);
    }
    __syncthreads();   // (the luma lanes store whole records, the chroma lanes then their bytes)
    if (!L.luma) {
      uint32_t l = 0, m, r = 0;
      if (b.here) {   // the pair's left block exists; its right block may not
        int x[16];
        fg_load_row<PIX>(fg_row_at(P, frames, L.plane, b.f, b.by, b.bx, L.row), b.both, x);
        fg_row_response(x, L.row > 0 && L.row < 7, l, m, r);
      }
      l = fg_sum_lanes(l, 8); r = fg_sum_lanes(r, 8);
      if (L.row == 0) {
        reinterpret_cast<uint8_t *>(rec)[L.slot * 4 + 1 + L.plane] = (uint8_t)av1mi_fg_value(l, 1, P.bit_depth);
        reinterpret_cast<uint8_t *>(rec)[(L.slot + 1) * 4 + 1 + L.plane] = (uint8_t)av1mi_fg_value(r, 1, P.bit_depth);
      }
    }
    __syncthreads();
    if (t < AV1MI_FG_WALK_SLOTS) {
      const Av1miFgSpot o = av1mi_fg_walk_spot(step, t, P.n_frames, nbx, nby);
      if (o.here) blocks[((size_t)o.f * nby + o.by) * nbx + o.bx] = rec[t];
    }
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
                                                                    Av1miFgBits bits) {
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
    quart[t] = (uint8_t)value[t];   // before the fill and the ceiling: what fg_ar_kernel.hip calls a block flat by
  }
  __syncthreads();
  if (!hdr_blob) return;
  for (int f = t; f < P.n_frames; f += FG_TABLE_THREADS)   // one writer per header
    fg_put_points(hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes, av1mi_frame_is_inter(P, f) ? bits.fg_inter : bits.fg_key, final_v);
}

}  // namespace

extern "C" hipError_t av1mi_launch_film_grain(const Av1miDevParams *P, const void *frames, Av1miFgBlock fg, int ceil_y, int ceil_c, uint8_t *hdr_blob,
                                              Av1miFgBits bits, hipStream_t stream) {
  if (P->n_frames < 1 || (((uintptr_t)frames | (uintptr_t)fg.blocks | (uintptr_t)fg.parts) & 15) || (hdr_blob && (bits.fg_key <= 0 || bits.fg_inter <= 0))) return hipErrorInvalidValue;
  const int nbx = av1mi_fg_blocks(P->true_w), nby = av1mi_fg_blocks(P->true_h);
  const size_t n = (size_t)P->n_frames * nbx * nby;
  if (n) {   // (a picture smaller than a block has none: the table is all 0)
    const long n_steps = av1mi_fg_walk_steps(P->n_frames, nbx, nby);
    const dim3 grid((unsigned)(n_steps < 4096 ? n_steps : 4096)), threads(AV1MI_FG_WALK_THREADS);
    if (P->bit_depth == 8) hipLaunchKernelGGL((fg_block_kernel<uint8_t>), grid, threads, 0, stream, *P, (const uint8_t *)frames, fg.blocks);
    else hipLaunchKernelGGL((fg_block_kernel<uint16_t>), grid, threads, 0, stream, *P, (const uint16_t *)frames, fg.blocks);
  }
  // the histograms in parts of at least FG_PART_RECORDS records, at most AV1MI_FG_PARTS of them; every part's slice starts on a 16-byte boundary
  size_t n_parts = (n + FG_PART_RECORDS - 1) / FG_PART_RECORDS;
  if (n_parts > AV1MI_FG_PARTS) n_parts = AV1MI_FG_PARTS;
  if (n_parts) {
    const size_t per = ((n + n_parts - 1) / n_parts + 3) & ~(size_t)3;
    n_parts = (n + per - 1) / per;
    hipLaunchKernelGGL(fg_hist_kernel, dim3((unsigned)n_parts), dim3(FG_TABLE_THREADS), 0, stream, (const uint32_t *)fg.blocks, n, per, fg.parts);
  }
  hipLaunchKernelGGL(fg_table_kernel, dim3(1), dim3(FG_TABLE_THREADS), 0, stream, *P, (const uint32_t *)fg.parts, (int)n_parts, ceil_y, ceil_c, fg.table,
                     fg.counts, fg.quart, hdr_blob, bits);
  return hipGetLastError();
}
