// fg_ar_kernel.hip - the film grain's autoregressive coefficients fitted to a chunk's source (av1mi_params.film_grain bits 12-13; DESIGN.md
// §3 item 7d; fg_ar_rule.h is the rule).  Two kernels on the main stream, behind fg_table_kernel and in front of the denoiser:
//
// fg_ar_sums_kernel: walks the estimate's block records in fg_block_kernel's order - a workgroup of three waves takes four pairs of
// blocks a step, waves 0 and 1 their eight luma blocks, wave 2 the four U and four V pair-rows - and skips a step's blocks that are no
// candidates by their record (a wave none of whose blocks is one does nothing).  LANES ARE POSITIONS, the offsets are registers: a
// lane holds one row of 16 samples, loaded with 16 bytes a load as fg_block_kernel does (a luma block's row, or the U (V) row of a pair of
// blocks), so a block's rows sit in consecutive lanes.  S, A and B meet by exchanges over the block's 16 (8) lanes, e stays in the lane's
// registers, the energy condition is tested the same way, and a block that fails it has its e zeroed rather than its lanes branched
// away.  The products of a row with the rows 1 .. L below it come from those lanes, two 16-bit residuals per 32-bit exchange; per offset
// the row's up to 16 products are summed in 32 bits with 24-bit multiply-adds (|e| < 2^14 and any sum of a flat block's products is at
// most its sum of e^2 < 2^28: fg_ar_rule.h) and added to the lane's 64-bit accumulator of that offset, 46 of them, kept across all of the
// workgroup's blocks.  Why not lanes as offsets: 46 of 64 lanes would work, every one of them would read the whole block - from LDS,
// where the 46 lanes of an offset row read addresses one word apart at best and the same words over and over - and the products of a lane
// would need 64-bit adds each.  With lanes as rows the block is read once into registers, LDS is not used in the loop at all and the
// inner loop is one full-rate instruction per product; the price is 92 accumulator registers - 202 VGPRs in all, two waves a SIMD,
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

constexpr int FGAR_THREADS = 192;
constexpr int FGAR_GROUP_WORDS = 3 * AV1MI_FGAR_PART;   // what a workgroup stores

__device__ __forceinline__ unsigned long long fgar_sum_lanes(unsigned long long v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
  for (int j = 0; j < 8; j++) pk[j] = ((uint32_t)e[2 * j] & 0xFFFFu) | ((uint32_t)e[2 * j + 1] << 16);
#pragma unroll
  for (int dy = 1; dy <= AV1MI_FGAR_MAX_LAG; dy++)
    if (dy <= lag) {
      const bool in = row + dy < N;
      int nb[16];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        uint32_t v = __shfl_down(pk[j], dy, 64);
        v = in ? v : 0u;
        nb[2 * j] = (int)(int16_t)(v & 0xFFFFu);
        nb[2 * j + 1] = (int)v >> 16;
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

template <typename PIX>
__global__ void __launch_bounds__(FGAR_THREADS) fg_ar_sums_kernel(Av1miDevParams P, const PIX *__restrict__ frames, const uint32_t *__restrict__ blocks,
                                                                  const uint8_t *__restrict__ quart, const uint32_t *__restrict__ counts, int lag,
                                                                  long long *__restrict__ parts) {
  __shared__ int q_of[AV1MI_FG_TABLE];
  __shared__ uint32_t n_of[AV1MI_FG_TABLE];
  __shared__ long long red[6][AV1MI_FGAR_PART];   // the half-waves' sums: four of luma, U, V
  const int t = threadIdx.x;
  if (t < AV1MI_FG_TABLE) { q_of[t] = quart[t]; n_of[t] = counts[t]; }
  __syncthreads();
  const int nbx = av1mi_fg_blocks(P.true_w), nby = av1mi_fg_blocks(P.true_h), npx = (nbx + 1) / 2;
  const long n_pairs = (long)P.n_frames * nby * npx, n_steps = (n_pairs + 3) / 4;
  const bool luma = t < 128;   // wave-uniform
  const int slot = luma ? t >> 4 : ((t >> 3) & 3) * 2, row = luma ? t & 15 : t & 7, plane = luma ? 0 : 1 + ((t - 128) >> 5);
  long long acc[AV1MI_FGAR_SUMS];
#pragma unroll
  for (int k = 0; k < AV1MI_FGAR_SUMS; k++) acc[k] = 0;
  long long n_flat = 0;
  for (long step = blockIdx.x; step < n_steps; step += gridDim.x) {
    // this lane's block (chroma: the left block of its pair), as fg_block_kernel places them
    const long gp = step * 4 + (slot >> 1);
    const int f = (int)(gp / ((long)nby * npx)), in_frame = (int)(gp % ((long)nby * npx));
    const int by = in_frame / npx, bx = (in_frame % npx) * 2 + (slot & 1);
    const bool here = gp < n_pairs && bx < nbx;
    const size_t at = ((size_t)f * nby + by) * nbx + bx;
    if (luma) {
      bool cand = false;
      int q = 0;
      if (here) {
        const uint32_t rec = blocks[at];
        cand = av1mi_fgar_candidate(rec, 0, q_of, n_of);
        q = q_of[rec & 7u];
      }
      if (!__ballot(cand)) continue;
      int x[16], S = 0, A = 0;
#pragma unroll
      for (int c = 0; c < 16; c++) x[c] = 0;
      if (cand) fg_load_row<PIX>(frames + (size_t)f * P.frame_samples + (size_t)(by * 16 + row) * P.stride_y + bx * 16, true, x);
#pragma unroll
      for (int c = 0; c < 16; c++) { S += x[c]; A += (2 * c - 15) * x[c]; }
      int B = (2 * row - 15) * S;
      for (int o = 8; o > 0; o >>= 1) { S += __shfl_xor(S, o, 64); A += __shfl_xor(A, o, 64); B += __shfl_xor(B, o, 64); }
      int e[16];
      unsigned long long en = 0;
#pragma unroll
      for (int c = 0; c < 16; c++) {
        e[c] = cand ? av1mi_fgar_residual(16, x[c], row, c, S, A, B) : 0;
        const uint32_t a = (uint32_t)(e[c] < 0 ? -e[c] : e[c]);   // (below 2^16: fg_ar_rule.h)
        en += a * a;
      }
      en = fgar_sum_lanes(en, 16);
      const bool flat = cand && av1mi_fgar_energy_ok(en, 16, q, P.bit_depth);
#pragma unroll
      for (int c = 0; c < 16; c++) e[c] = flat ? e[c] : 0;
      if (flat && row == 0) n_flat++;
      if (__ballot(flat)) fgar_accumulate<16>(e, row, lag, acc);
    } else {
      bool cand[2] = { false, false };
      int q[2] = { 0, 0 };
      const bool both = here && bx + 1 < nbx;
      if (here) {
        const uint32_t rec = blocks[at];
        cand[0] = av1mi_fgar_candidate(rec, plane, q_of + plane * AV1MI_FG_BINS, n_of + plane * AV1MI_FG_BINS);
        q[0] = q_of[plane * AV1MI_FG_BINS + (rec & 7u)];
      }
      if (both) {
        const uint32_t rec = blocks[at + 1];
        cand[1] = av1mi_fgar_candidate(rec, plane, q_of + plane * AV1MI_FG_BINS, n_of + plane * AV1MI_FG_BINS);
        q[1] = q_of[plane * AV1MI_FG_BINS + (rec & 7u)];
      }
      if (!__ballot(cand[0] || cand[1])) continue;
      int x[16], S[2] = { 0, 0 }, A[2] = { 0, 0 }, B[2];
#pragma unroll
      for (int c = 0; c < 16; c++) x[c] = 0;
      if (cand[0] || cand[1])
        fg_load_row<PIX>(frames + (size_t)f * P.frame_samples + (plane == 1 ? P.plane_off_u : P.plane_off_v) + (size_t)(by * 8 + row) * P.stride_c + bx * 8, both, x);
#pragma unroll
      for (int c = 0; c < 16; c++) { S[c >> 3] += x[c]; A[c >> 3] += (2 * (c & 7) - 7) * x[c]; }
      B[0] = (2 * row - 7) * S[0]; B[1] = (2 * row - 7) * S[1];
      for (int o = 4; o > 0; o >>= 1)
#pragma unroll
        for (int h = 0; h < 2; h++) { S[h] += __shfl_xor(S[h], o, 64); A[h] += __shfl_xor(A[h], o, 64); B[h] += __shfl_xor(B[h], o, 64); }
      int e[16];
      unsigned long long en[2] = { 0, 0 };
#pragma unroll
      for (int c = 0; c < 16; c++) {
        e[c] = cand[c >> 3] ? av1mi_fgar_residual(8, x[c], row, c & 7, S[c >> 3], A[c >> 3], B[c >> 3]) : 0;
        const uint32_t a = (uint32_t)(e[c] < 0 ? -e[c] : e[c]);
        en[c >> 3] += a * a;
      }
      bool flat[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        en[h] = fgar_sum_lanes(en[h], 8);
        flat[h] = cand[h] && av1mi_fgar_energy_ok(en[h], 8, q[h], P.bit_depth);
        if (flat[h] && row == 0) n_flat++;
      }
#pragma unroll
      for (int c = 0; c < 16; c++) e[c] = flat[c >> 3] ? e[c] : 0;
      if (__ballot(flat[0] || flat[1])) fgar_accumulate<8>(e, row, lag, acc);
    }
  }
  // the lanes' sums over each half-wave (a plane's lanes fill whole half-waves), then over the workgroup per plane
#pragma unroll
  for (int k = 0; k < AV1MI_FGAR_SUMS; k++) {
    const long long v = (long long)fgar_sum_lanes((unsigned long long)acc[k], 32);
    if ((t & 31) == 0) red[t >> 5][k] = v;
  }
  n_flat = (long long)fgar_sum_lanes((unsigned long long)n_flat, 32);
  if ((t & 31) == 0) red[t >> 5][AV1MI_FGAR_SUMS] = n_flat;
  __syncthreads();
  if (t < FGAR_GROUP_WORDS) {
    const int pl = t / AV1MI_FGAR_PART, k = t % AV1MI_FGAR_PART;
    parts[(size_t)blockIdx.x * FGAR_GROUP_WORDS + t] = pl == 0 ? red[0][k] + red[1][k] + red[2][k] + red[3][k] : red[3 + pl][k];
  }
}

constexpr int FGAR_SOLVE_THREADS = 1024, FGAR_SLICES = 7, FGAR_SLICE_STRIDE = 144;   // 7 x 144 lanes sum the parts

__global__ void __launch_bounds__(FGAR_SOLVE_THREADS) fg_ar_solve_kernel(Av1miDevParams P, const long long *__restrict__ parts, int n_groups, int lag,
                                                                         const uint8_t *__restrict__ table, uint8_t *__restrict__ out,
                                                                         uint8_t *__restrict__ hdr_blob, int fg_bit_key, int fg_bit_inter, int ar_bit_key,
                                                                         int ar_bit_inter) {
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
    out[AV1MI_FGAR_TABLE_AT + t] = (uint8_t)v;
    out[AV1MI_FGAR_SIGMA_AT + t] = table[t];
  }
  if (t < 3 * AV1MI_FGAR_COEFFS) out[AV1MI_FGAR_COEFF_AT + t] = (uint8_t)coef[t / AV1MI_FGAR_COEFFS][t % AV1MI_FGAR_COEFFS];
  if (t < 3) {
    reinterpret_cast<uint32_t *>(out + AV1MI_FGAR_GAIN_AT)[t] = gain[t];
    reinterpret_cast<uint32_t *>(out + AV1MI_FGAR_FLAT_AT)[t] = (uint32_t)sums[t * AV1MI_FGAR_PART + AV1MI_FGAR_SUMS];
  }
  if (t < 3 * AV1MI_FGAR_SUMS) reinterpret_cast<long long *>(out + AV1MI_FGAR_SUMS_AT)[t] = sums[(t / AV1MI_FGAR_SUMS) * AV1MI_FGAR_PART + t % AV1MI_FGAR_SUMS];
  __syncthreads();
  if (!hdr_blob) return;
  const int n_pos = av1mi_fgar_positions(lag);
  for (int f = t; f < P.n_frames; f += FGAR_SOLVE_THREADS) {   // one writer per header
    uint8_t *h = hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
    const bool inter = av1mi_frame_is_inter(P, f);
    const int bit = inter ? fg_bit_inter : fg_bit_key;
    for (int pl = 0; pl < 3; pl++)
      for (int k = 0; k < AV1MI_FG_BINS; k++)
        av1mi_fg_put8(h, bit + (pl == 0 ? 0 : (pl == 1 ? AV1MI_FG_CB_BIT : AV1MI_FG_CR_BIT)) + 16 * k + 8, (uint32_t)final_v[pl * AV1MI_FG_BINS + k]);
    int ar = inter ? ar_bit_inter : ar_bit_key;
    for (int pl = 0; pl < 3; pl++)   // luma's positions, then cb's and cr's with their luma tap (0) behind them
      for (int i = 0; i < n_pos + (pl ? 1 : 0); i++, ar += 8) av1mi_fg_put8(h, ar, (uint32_t)(128 + (i < n_pos ? coef[pl][i] : 0)));
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_fg_ar(const Av1miDevParams *P, const void *frames, const uint32_t *blocks, const uint8_t *quart, const uint32_t *counts,
                                         const uint8_t *table, int lag, uint8_t *ar, uint8_t *hdr_blob, int fg_bit_key, int fg_bit_inter, int ar_bit_key,
                                         int ar_bit_inter, hipStream_t stream) {
  if (P->n_frames < 1 || lag < 1 || lag > AV1MI_FGAR_MAX_LAG || ((uintptr_t)frames & 15) || ((uintptr_t)ar & 15) ||
      (hdr_blob && (fg_bit_key <= 0 || fg_bit_inter <= 0 || ar_bit_key <= 0 || ar_bit_inter <= 0)))
    return hipErrorInvalidValue;
  const int nbx = av1mi_fg_blocks(P->true_w), nby = av1mi_fg_blocks(P->true_h);
  const long n_steps = ((long)P->n_frames * nby * ((nbx + 1) / 2) + 3) / 4;
  const int n_groups = (int)(n_steps < AV1MI_FGAR_MAX_GROUPS ? n_steps : AV1MI_FGAR_MAX_GROUPS);
  long long *parts = reinterpret_cast<long long *>(ar + AV1MI_FGAR_RESULT_BYTES);
  if (n_groups) {   // (a picture smaller than a block has none: no fit)
    if (P->bit_depth == 8) hipLaunchKernelGGL((fg_ar_sums_kernel<uint8_t>), dim3((unsigned)n_groups), dim3(FGAR_THREADS), 0, stream, *P, (const uint8_t *)frames, blocks, quart, counts, lag, parts);
    else hipLaunchKernelGGL((fg_ar_sums_kernel<uint16_t>), dim3((unsigned)n_groups), dim3(FGAR_THREADS), 0, stream, *P, (const uint16_t *)frames, blocks, quart, counts, lag, parts);
  }
  hipLaunchKernelGGL(fg_ar_solve_kernel, dim3(1), dim3(FGAR_SOLVE_THREADS), 0, stream, *P, (const long long *)parts, n_groups, lag, table, ar, hdr_blob,
                     fg_bit_key, fg_bit_inter, ar_bit_key, ar_bit_inter);
  return hipGetLastError();
}
