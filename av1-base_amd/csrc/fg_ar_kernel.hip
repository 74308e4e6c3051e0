// fg_ar_kernel.hip - the film grain's autoregressive coefficients fitted to a chunk's source (av1mi_params.film_grain bits 12-13; DESIGN.md
// §3 item 7d; fg_ar_rule.h is the rule).  Two kernels on the main stream, behind fg_table_kernel and in front of the denoiser:
//
// fg_ar_sums_kernel: walks the estimate's block records by fg_rule.h's block walk, the code fg_block_kernel wrote them by - a workgroup of
// three waves takes four pairs of blocks a step, waves 0 and 1 their eight luma blocks, wave 2 the four U and four V pair-rows - and skips
// a step's blocks that are no candidates by their record (a wave none of whose blocks is one does nothing).  One body, fgar_step<N>, for
// the luma waves (N = 16, one block per lane row) and the chroma wave (N = 8, two).  LANES ARE POSITIONS, the offsets are registers: a
// lane holds one row of 16 samples, addressed, loaded, packed and summed with fg_pieces.h's pieces as fg_block_kernel does, so a block's
// rows sit in consecutive lanes.  S, A and B meet by exchanges over the block's 16 (8) lanes, e stays in the lane's
// registers, the energy condition is tested the same way, and a block that fails it has its e zeroed rather than its lanes branched
// away.  The products of a row with the rows 1 .. L below it come from those lanes, two 16-bit residuals per 32-bit exchange; per offset
// the row's up to 16 products are summed in 32 bits with 24-bit multiply-adds (|e| < 2^14 and any sum of a flat block's products is at
// most its sum of e^2 < 2^28: fg_ar_rule.h) and added to the lane's 64-bit accumulator of that offset, 46 of them, kept across all of the
// workgroup's blocks.  Why not lanes as offsets: 46 of 64 lanes would work, every one of them would read the whole block - from LDS,
// where the 46 lanes of an offset row read addresses one word apart at best and the same words over and over - and the products of a lane
// would need 64-bit adds each.  With lanes as rows the block is read once into registers, LDS is not used in the loop at all and the
// inner loop is one full-rate instruction per product; the price is 92 accumulator registers - 198 VGPRs in all, two waves a SIMD,
// no scratch - in a loop with one load per step and otherwise arithmetic.  At the end the accumulators are reduced
// over the lanes of a plane and the workgroup stores its part: store and sum, no atomics; integer sums, so any grid gives the same.
// Algorithmic HBM bytes: the candidate blocks' samples once (at most n L b 3 / 2, L luma samples of the counted blocks, b bytes each)
// plus the records, 4 n L / 256, plus 1128 bytes per workgroup.
// fg_ar_solve_kernel: one workgroup.  The parts' sum, then per plane the rule's steps 4 - 6 - the correlations one lane each, the solve one
// lane per plane in waves of their own on LDS - the result block (coefficients, both tables, gains, flat blocks, sums), and into every
// frame's header slot the coefficient bytes at fg_ar_bit and the scaled points at fg_bit, one lane per header.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "fg_ar_rule.h"
#include "fg_pieces.h"

namespace {

constexpr int FGAR_GROUP_WORDS = 3 * AV1MI_FGAR_PART;   // what a workgroup stores

// the products of this lane's row e[] - 16 / N blocks' rows of N residuals - with itself and with the rows 1 .. lag below it (the lanes
// behind this one, while they are rows of the same blocks), added to acc[]; every lane of the wave comes here
template <int N>
__device__ __forceinline__ void fgar_accumulate(const int (&e)[16], int row, int lag, long long (&acc)[AV1MI_FGAR_SUMS]) {
#pragma unroll
  for (int dx = 0; dx <= 2 * AV1MI_FGAR_MAX_LAG; dx++)
    if (dx <= 2 * lag) {
      int s = 0;
#pragma unroll
      for (int c = 0; c < 16; c++)
        if ((c & (N - 1)) + dx < N) s += __mul24(e[c], e[(c + dx) & 15]);
      acc[av1mi_fgar_index(0, dx)] += s;
    }
  uint32_t pk[8];
#pragma unroll
  for (int j = 0; j < 8; j++) pk[j] = fg_pack2(e[2 * j], e[2 * j + 1]);
#pragma unroll
  for (int dy = 1; dy <= AV1MI_FGAR_MAX_LAG; dy++)
    if (dy <= lag) {
      const bool in = row + dy < N;
      int nb[16];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        uint32_t v = __shfl_down(pk[j], dy, 64);
        v = in ? v : 0u;
        nb[2 * j] = fg_lo16(v);
        nb[2 * j + 1] = fg_hi16(v);
      }
#pragma unroll
      for (int dx = -2 * AV1MI_FGAR_MAX_LAG; dx <= 2 * AV1MI_FGAR_MAX_LAG; dx++)
        if ((dx < 0 ? -dx : dx) <= 2 * lag) {
          int s = 0;
#pragma unroll
          for (int c = 0; c < 16; c++)
            if ((c & (N - 1)) + dx >= 0 && (c & (N - 1)) + dx < N) s += __mul24(e[c], nb[(c + dx) & 15]);
          acc[av1mi_fgar_index(dy, dx)] += s;
        }
    }
}

// One step of a wave's lanes, all 64 of which come here: a lane's row holds H blocks' rows of N samples, spot b's block and (chroma) the one
// right of it.  A block that is no candidate by its record, or is not there, stays all zero: nothing of it is loaded (`both` guards the
// right record and the right 8 samples) and its e[] adds nothing.  Returns early only when no lane of the wave has a candidate (a
// ballot: wave-uniform), so every exchange below is reached by all lanes; no barrier in here.
template <int N, typename PIX>
__device__ __forceinline__ void fgar_step(const Av1miDevParams &P, const PIX *frames, const uint32_t *blocks, size_t at, const Av1miFgSpot &b, int plane, int row,
                                          const int *q_of, const uint32_t *n_of, int lag, long long (&acc)[AV1MI_FGAR_SUMS], long long &n_flat) {
  constexpr int H = 16 / N;
  bool cand[H], flat[H], any = false;
  int q[H], S[H], A[H], B[H];
  unsigned long long en[H];
#pragma unroll
  for (int h = 0; h < H; h++) {
    cand[h] = false; q[h] = S[h] = A[h] = 0; en[h] = 0;
    if (h ? b.both : b.here) {
      const uint32_t rec = blocks[at + h];
      cand[h] = av1mi_fgar_candidate(rec, plane, q_of + plane * AV1MI_FG_BINS, n_of + plane * AV1MI_FG_BINS);
      q[h] = q_of[plane * AV1MI_FG_BINS + (rec & 7u)];
    }
    any = any || cand[h];
  }
  if (!__ballot(any)) return;
  int x[16], e[16];
#pragma unroll
  for (int c = 0; c < 16; c++) x[c] = 0;
  if (any) fg_load_row<PIX>(fg_row_at(P, frames, plane, b.f, b.by, b.bx, row), N == 16 || b.both, x);
#pragma unroll
  for (int c = 0; c < 16; c++) { S[c / N] += x[c]; A[c / N] += (2 * (c & (N - 1)) - (N - 1)) * x[c]; }
#pragma unroll
  for (int h = 0; h < H; h++) {
    B[h] = (2 * row - (N - 1)) * S[h];
    S[h] = fg_sum_lanes(S[h], N); A[h] = fg_sum_lanes(A[h], N); B[h] = fg_sum_lanes(B[h], N);
  }
#pragma unroll
  for (int c = 0; c < 16; c++) {
    e[c] = cand[c / N] ? av1mi_fgar_residual(N, x[c], row, c & (N - 1), S[c / N], A[c / N], B[c / N]) : 0;
    const uint32_t a = (uint32_t)(e[c] < 0 ? -e[c] : e[c]);   // (below 2^16: fg_ar_rule.h)
    en[c / N] += a * a;
  }
  any = false;
#pragma unroll
  for (int h = 0; h < H; h++) {
    en[h] = fg_sum_lanes(en[h], N);
    flat[h] = cand[h] && av1mi_fgar_energy_ok(en[h], N, q[h], P.bit_depth);
    if (flat[h] && row == 0) n_flat++;
    any = any || flat[h];
  }
#pragma unroll
  for (int c = 0; c < 16; c++) e[c] = flat[c / N] ? e[c] : 0;
  if (__ballot(any)) fgar_accumulate<N>(e, row, lag, acc);
}

template <typename PIX>
__global__ void __launch_bounds__(AV1MI_FG_WALK_THREADS) fg_ar_sums_kernel(Av1miDevParams P, const PIX *__restrict__ frames, const uint32_t *__restrict__ blocks,
                                                                           const uint8_t *__restrict__ quart, const uint32_t *__restrict__ counts, int lag,
                                                                           long long *__restrict__ parts) {
  __shared__ int q_of[AV1MI_FG_TABLE];
  __shared__ uint32_t n_of[AV1MI_FG_TABLE];
  __shared__ long long red[6][AV1MI_FGAR_PART];   // the half-waves' sums: four of luma, U, V
  const int t = threadIdx.x;
  if (t < AV1MI_FG_TABLE) { q_of[t] = quart[t]; n_of[t] = counts[t]; }
  __syncthreads();
  const int nbx = av1mi_fg_blocks(P.true_w), nby = av1mi_fg_blocks(P.true_h);
  const long n_steps = av1mi_fg_walk_steps(P.n_frames, nbx, nby);
  const Av1miFgLane L = av1mi_fg_walk_lane(t);
  long long acc[AV1MI_FGAR_SUMS];
#pragma unroll
  for (int k = 0; k < AV1MI_FGAR_SUMS; k++) acc[k] = 0;
  long long n_flat = 0;
  for (long step = blockIdx.x; step < n_steps; step += gridDim.x) {   // (no barrier in the loop: a wave without candidates goes on alone)
    const Av1miFgSpot b = av1mi_fg_walk_spot(step, L.slot, P.n_frames, nbx, nby);   // this lane's block (chroma: the left block of its pair)
    const size_t at = ((size_t)b.f * nby + b.by) * nbx + b.bx;
    if (L.luma) fgar_step<16, PIX>(P, frames, blocks, at, b, 0, L.row, q_of, n_of, lag, acc, n_flat);   // (wave-uniform)
    else fgar_step<8, PIX>(P, frames, blocks, at, b, L.plane, L.row, q_of, n_of, lag, acc, n_flat);
  }
  // the lanes' sums over each half-wave (a plane's lanes fill whole half-waves), then over the workgroup per plane
#pragma unroll
  for (int k = 0; k < AV1MI_FGAR_SUMS; k++) {
    const long long v = fg_sum_lanes(acc[k], 32);
    if ((t & 31) == 0) red[t >> 5][k] = v;
  }
  n_flat = fg_sum_lanes(n_flat, 32);
  if ((t & 31) == 0) red[t >> 5][AV1MI_FGAR_SUMS] = n_flat;
  __syncthreads();
  if (t < FGAR_GROUP_WORDS) {
    const int pl = t / AV1MI_FGAR_PART, k = t % AV1MI_FGAR_PART;
    parts[(size_t)blockIdx.x * FGAR_GROUP_WORDS + t] = pl == 0 ? red[0][k] + red[1][k] + red[2][k] + red[3][k] : red[3 + pl][k];
  }
}

constexpr int FGAR_SOLVE_THREADS = 1024, FGAR_SLICES = 7, FGAR_SLICE_STRIDE = 144;   // 7 x 144 lanes sum the parts

__global__ void __launch_bounds__(FGAR_SOLVE_THREADS) fg_ar_solve_kernel(Av1miDevParams P, const long long *__restrict__ parts, int n_groups, int lag,
                                                                         const uint8_t *__restrict__ table, Av1miFgArBlock out,
                                                                         uint8_t *__restrict__ hdr_blob, Av1miFgBits bits) {
  __shared__ long long slice[FGAR_SLICES][FGAR_SLICE_STRIDE];
  __shared__ long long sums[FGAR_GROUP_WORDS];
  __shared__ int rho[3 * AV1MI_FGAR_SUMS];
  __shared__ long long ws[3][AV1MI_FGAR_WS];
  __shared__ int8_t coef[3][AV1MI_FGAR_COEFFS];
  __shared__ uint32_t gain[3];
  __shared__ int final_v[AV1MI_FG_TABLE];
  const int t = threadIdx.x;
  {
    const int v = t % FGAR_SLICE_STRIDE, s = t / FGAR_SLICE_STRIDE;
    if (v < FGAR_GROUP_WORDS && s < FGAR_SLICES) {
      long long a = 0;
      for (int g = s; g < n_groups; g += FGAR_SLICES) a += parts[(size_t)g * FGAR_GROUP_WORDS + v];
      slice[s][v] = a;
    }
  }
  __syncthreads();
  if (t < FGAR_GROUP_WORDS) {
    long long a = 0;
    for (int s = 0; s < FGAR_SLICES; s++) a += slice[s][t];
    sums[t] = a;
  }
  __syncthreads();
  if (t < 3 * AV1MI_FGAR_SUMS) {   // the correlations, one lane each
    const int pl = t / AV1MI_FGAR_SUMS, k = t % AV1MI_FGAR_SUMS;
    const long long *R = sums + pl * AV1MI_FGAR_PART;
    const bool fit = R[AV1MI_FGAR_SUMS] >= AV1MI_FGAR_MIN_FLAT && R[0] > 0 && av1mi_fgar_index_used(k, lag);
    rho[t] = fit ? av1mi_fgar_rho(R, k, pl ? 8 : 16) : 0;
  }
  __syncthreads();
  if ((t & 63) == 0 && t < 3 * 64) {   // the planes' solves, in three waves
    const int pl = t >> 6;
    const long long *R = sums + pl * AV1MI_FGAR_PART;
    av1mi_fgar_fit(lag, R, (uint32_t)R[AV1MI_FGAR_SUMS], pl ? 8 : 16, rho + pl * AV1MI_FGAR_SUMS, true, ws[pl], coef[pl], &gain[pl]);
  }
  __syncthreads();
  if (t < AV1MI_FG_TABLE) {
    const int v = av1mi_fgar_compensate(table[t], gain[t / AV1MI_FG_BINS]);
    final_v[t] = v;
    out.table[t] = (uint8_t)v;
    out.sigma[t] = table[t];
  }
  if (t < 3 * AV1MI_FGAR_COEFFS) out.coeffs[t] = coef[t / AV1MI_FGAR_COEFFS][t % AV1MI_FGAR_COEFFS];
  if (t < 3) {
    out.gain[t] = gain[t];
    out.flat[t] = (uint32_t)sums[t * AV1MI_FGAR_PART + AV1MI_FGAR_SUMS];
  }
  if (t < 3 * AV1MI_FGAR_SUMS) out.sums[t] = sums[(t / AV1MI_FGAR_SUMS) * AV1MI_FGAR_PART + t % AV1MI_FGAR_SUMS];
  __syncthreads();
  if (!hdr_blob) return;
  const int n_pos = av1mi_fgar_positions(lag);
  for (int f = t; f < P.n_frames; f += FGAR_SOLVE_THREADS) {   // one writer per header
    uint8_t *h = hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
    const bool inter = av1mi_frame_is_inter(P, f);
    fg_put_points(h, inter ? bits.fg_inter : bits.fg_key, final_v);
    int ar = inter ? bits.ar_inter : bits.ar_key;
    for (int pl = 0; pl < 3; pl++)   // luma's positions, then cb's and cr's with their luma tap (0) behind them
      for (int i = 0; i < n_pos + (pl ? 1 : 0); i++, ar += 8) av1mi_fg_put8(h, ar, (uint32_t)(128 + (i < n_pos ? coef[pl][i] : 0)));
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_fg_ar(const Av1miDevParams *P, const void *frames, Av1miFgBlock fg, int lag, Av1miFgArBlock ar, uint8_t *hdr_blob,
                                         Av1miFgBits bits, hipStream_t stream) {
  if (P->n_frames < 1 || lag < 1 || lag > AV1MI_FGAR_MAX_LAG || ((uintptr_t)frames & 15) || ((uintptr_t)ar.coeffs & 15) ||
      (hdr_blob && (bits.fg_key <= 0 || bits.fg_inter <= 0 || bits.ar_key <= 0 || bits.ar_inter <= 0)))
    return hipErrorInvalidValue;
  const long n_steps = av1mi_fg_walk_steps(P->n_frames, av1mi_fg_blocks(P->true_w), av1mi_fg_blocks(P->true_h));
  const int n_groups = (int)(n_steps < AV1MI_FGAR_MAX_GROUPS ? n_steps : AV1MI_FGAR_MAX_GROUPS);
  const dim3 grid((unsigned)n_groups), threads(AV1MI_FG_WALK_THREADS);
  if (n_groups) {   // (a picture smaller than a block has none: no fit)
    if (P->bit_depth == 8) hipLaunchKernelGGL((fg_ar_sums_kernel<uint8_t>), grid, threads, 0, stream, *P, (const uint8_t *)frames, fg.blocks, fg.quart, fg.counts, lag, ar.parts);
    else hipLaunchKernelGGL((fg_ar_sums_kernel<uint16_t>), grid, threads, 0, stream, *P, (const uint16_t *)frames, fg.blocks, fg.quart, fg.counts, lag, ar.parts);
  }
  hipLaunchKernelGGL(fg_ar_solve_kernel, dim3(1), dim3(FGAR_SOLVE_THREADS), 0, stream, *P, (const long long *)ar.parts, n_groups, lag, fg.table, ar, hdr_blob, bits);
  return hipGetLastError();
}
