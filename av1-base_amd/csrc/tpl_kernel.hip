// tpl_kernel.hip - the temporal-dependency analysis behind the adaptive quantisation's temporal term (av1mi_params.cq_level bits 12-14;
// DESIGN.md §3 item 1d; tpl_rule.h is the rule; SURVEY.md §8a "look-ahead": what SVT-AV1 and libaom call TPL).  Open loop, from the
// SOURCE luma of a whole chunk, before any tile walk: how much of the frames that follow each 16x16 block is going to predict.
//
// tpl_cost_kernel: one wave per (block, frame).  The wave holds the block's rows in tf_search.h's layout, so it sums S, m and I with
// v_sad_u16 and the DPP row sum, and - inter frames only, a wave-uniform branch - runs the temporal filter's search against the frame
// before: I, C and the winner's node key per block.  tpl_flow_kernel: one launch per inter frame from the chunk's last frame down; a lane
// takes one block of frame f and adds its up to four shares into A[f - 1] with 64-bit integer atomics (any order gives the same sums).
// Stream order is the only dependency between the frames' launches.  tpl_beta_kernel: one wave per (superblock, frame), lane = 16x16
// block of the superblock: O, P, beta, and beta added into the chunk's sum, from which aq_map_kernel (scene_kernels.hip) takes Mb.
// tpl_frame_kernel (the frame term, cq_level bits 20-22): one workgroup per frame sums I and I + A over the frame's blocks and beta over
// its superblocks - 64 bits per lane, a wave reduction, one LDS step, no atomics - and leaves OF, PF, betaF and the sum of beta per frame,
// from which aq_map_kernel takes the frames' indices.
// Algorithmic HBM bytes per chunk of n frames: 2 n L b read by the search (L luma samples, b bytes each; the 2R+1-fold re-reads are L1 /
// L2 hits), 12 n L / 256 written by it, and about 56 n L / 256 moved by the flow and the superblock pass.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "tf_search.h"
#include "tpl_rule.h"

namespace {

template <typename PIX, int R>
__global__ void __launch_bounds__(64) tpl_cost_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ intra,
                                                      uint32_t *__restrict__ inter, uint32_t *__restrict__ key) {
  const int W = P.width, H = P.height, nbx = av1mi_tpl_blocks(W), nb = nbx * av1mi_tpl_blocks(H);
  const int b = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  const PIX *cur = frames + (size_t)f * P.frame_samples;   // luma of frame f; an inter frame has frame f - 1 in front of it
  const int x = (b % nbx) * AV1MI_TPL_BLOCK, y = (b / nbx) * AV1MI_TPL_BLOCK;
  const bool is_inter = av1mi_frame_is_inter(P, f);   // wave-uniform
  uint32_t s2[8], k = AV1MI_ME_NODE_NONE;
  if (is_inter) k = tf_search_block<PIX, R>(cur, cur - P.frame_samples, x, y, W, H, P.stride_y, lane, s2);
  else tf_block_row<PIX>(cur, x, y, W, H, P.stride_y, lane, s2);
  // S over the block: the pairs against zero, then over the 16 rows; I likewise against m in both halves
  uint32_t a = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) a = __builtin_amdgcn_sad_u16(s2[i], 0u, a);
  const uint32_t m = av1mi_tpl_mean(tf_row_sum_u32(a)), mm = m | (m << 16);
  a = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) a = __builtin_amdgcn_sad_u16(s2[i], mm, a);
  const uint32_t I = av1mi_tpl_intra(tf_row_sum_u32(a));
  uint32_t C = I;
  if (is_inter) {
    const int NC = 2 * R + 1, idx = (int)av1mi_me_node_index(k), dy = idx / NC - R, dx = idx % NC - R;
    C = av1mi_tpl_inter(av1mi_me_node_cost(k) - (uint32_t)(AV1MI_TPL_BLOCK * (av1mi_me_iabs(dx) + av1mi_me_iabs(dy))), I);
  }
  if (lane == 0) {
    const size_t at = (size_t)f * nb + b;
    intra[at] = I; inter[at] = C; key[at] = k;
  }
}

// frame f (an inter frame) hands its blocks' T to frame f - 1
__global__ void __launch_bounds__(256) tpl_flow_kernel(const uint32_t *__restrict__ intra, const uint32_t *__restrict__ inter, const uint32_t *__restrict__ key,
                                                       unsigned long long *__restrict__ flow, int nbx, int nby, int R, int f) {
  const int nb = nbx * nby, b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const size_t at = (size_t)f * nb + b;
  const uint32_t I = intra[at], C = inter[at];
  if (C >= I) return;   // T = 0
  const uint64_t T = av1mi_tpl_flow(I, C, flow[at]);
  const int NC = 2 * R + 1, idx = (int)av1mi_me_node_index(key[at]), dy = idx / NC - R, dx = idx % NC - R;
  unsigned long long *to = flow + (size_t)(f - 1) * nb;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint64_t share;
    const int cell = av1mi_tpl_part(k, b % nbx, b / nbx, dx, dy, nbx, nby, T, &share);
    if (cell >= 0 && share) atomicAdd(to + cell, (unsigned long long)share);
  }
}

// beta of every superblock; sum: the chunk's sum of beta (zeroed by the caller)
__global__ void __launch_bounds__(64) tpl_beta_kernel(Av1miDevParams P, const uint32_t *__restrict__ intra, const unsigned long long *__restrict__ flow,
                                                      uint16_t *__restrict__ beta, unsigned long long *__restrict__ sum) {
  const int nbx = av1mi_tpl_blocks(P.width), nby = av1mi_tpl_blocks(P.height), nb = nbx * nby;
  const int sb = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  const int bx = (sb % P.sb_cols) * 4 + (lane & 3), by = (sb / P.sb_cols) * 4 + ((lane >> 2) & 3);
  unsigned long long O = 0, Pv = 0;
  if (lane < 16 && bx < nbx && by < nby) {
    const size_t at = (size_t)f * nb + (size_t)by * nbx + bx;
    O = intra[at]; Pv = O + flow[at];
  }
  for (int o = 8; o > 0; o >>= 1) { O += __shfl_xor(O, o, 64); Pv += __shfl_xor(Pv, o, 64); }
  if (lane == 0) {   // (the superblock's first block is inside the grid: O >= 1)
    const int v = av1mi_tpl_beta(O, Pv);
    beta[(size_t)f * P.sb_rows * P.sb_cols + sb] = (uint16_t)v;
    if (v) atomicAdd(sum, (unsigned long long)v);
  }
}

// the frame's sums (tpl_rule.h "frame"): OF, PF, betaF and the sum of beta over the frame's superblocks, behind tpl_beta_kernel
__global__ void __launch_bounds__(256) tpl_frame_kernel(Av1miDevParams P, const uint32_t *__restrict__ intra, const unsigned long long *__restrict__ flow,
                                                        const uint16_t *__restrict__ beta, Av1miFqBlock out) {
  __shared__ unsigned long long part[3][4];
  const int nb = av1mi_tpl_blocks(P.width) * av1mi_tpl_blocks(P.height), nsb = P.sb_rows * P.sb_cols;
  const int f = blockIdx.x, t = threadIdx.x;
  unsigned long long O = 0, Pv = 0, B = 0;
  for (int i = t; i < nb; i += 256) {
    const size_t at = (size_t)f * nb + i;
    const unsigned long long I = intra[at];
    O += I; Pv += I + flow[at];
  }
  for (int i = t; i < nsb; i += 256) B += beta[(size_t)f * nsb + i];
  for (int o = 32; o > 0; o >>= 1) { O += __shfl_xor(O, o, 64); Pv += __shfl_xor(Pv, o, 64); B += __shfl_xor(B, o, 64); }
  if ((t & 63) == 0) { part[0][t >> 6] = O; part[1][t >> 6] = Pv; part[2][t >> 6] = B; }
  __syncthreads();
  if (t == 0) {   // (every block has I >= 1: OF >= 1)
    O = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    Pv = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    out.intra_sum[f] = O; out.dep_sum[f] = Pv;
    out.sb_beta_sum[f] = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    out.beta[f] = (uint16_t)av1mi_fq_beta(O, Pv);
  }
}

template <typename PIX>
hipError_t launch_tpl(const Av1miDevParams &P, const void *frames, uint32_t *intra, uint32_t *inter, uint32_t *key, unsigned long long *flow,
                      uint16_t *beta, hipStream_t stream) {
  const int nbx = av1mi_tpl_blocks(P.width), nby = av1mi_tpl_blocks(P.height), nb = nbx * nby;
  const dim3 gc(nb, P.n_frames);
  if (P.me_range == 16) hipLaunchKernelGGL((tpl_cost_kernel<PIX, 16>), gc, dim3(64), 0, stream, P, (const PIX *)frames, intra, inter, key);
  else hipLaunchKernelGGL((tpl_cost_kernel<PIX, 8>), gc, dim3(64), 0, stream, P, (const PIX *)frames, intra, inter, key);
  for (int f = P.n_frames - 1; f > 0; f--)
    if (av1mi_frame_is_inter(P, f))
      hipLaunchKernelGGL(tpl_flow_kernel, dim3((nb + 255) / 256), dim3(256), 0, stream, (const uint32_t *)intra, (const uint32_t *)inter, (const uint32_t *)key, flow,
                         nbx, nby, P.me_range, f);
  hipLaunchKernelGGL(tpl_beta_kernel, dim3(P.sb_rows * P.sb_cols, P.n_frames), dim3(64), 0, stream, P, (const uint32_t *)intra,
                     (const unsigned long long *)flow, beta, flow + av1mi_tpl_flow_entries(P.width, P.height, P.n_frames) - 1);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t av1mi_launch_tpl(const Av1miDevParams *P, const void *frames, uint32_t *intra, uint32_t *inter, uint32_t *key,
                                       unsigned long long *flow, uint16_t *beta, hipStream_t stream) {
  if ((P->me_range != 8 && P->me_range != 16) || P->keyint < 1 || P->n_frames < 1 || ((uintptr_t)frames & 15)) return hipErrorInvalidValue;
  return P->bit_depth == 8 ? launch_tpl<uint8_t>(*P, frames, intra, inter, key, flow, beta, stream)
                           : launch_tpl<uint16_t>(*P, frames, intra, inter, key, flow, beta, stream);
}

extern "C" hipError_t av1mi_launch_tpl_frames(const Av1miDevParams *P, const uint32_t *intra, const unsigned long long *flow, const uint16_t *beta,
                                              Av1miFqBlock fq, hipStream_t stream) {
  if (P->n_frames < 1 || !intra || !flow || !beta || !fq.intra_sum) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tpl_frame_kernel, dim3(P->n_frames), dim3(256), 0, stream, *P, intra, flow, beta, fq);
  return hipGetLastError();
}
