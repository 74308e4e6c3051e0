// tf_kernel.hip - the key frames' temporal filter (av1mi_params.me_presearch bits 8-14; SURVEY.md §8a
// "look-ahead": SVT-AV1 codes a motion-compensated temporal filter of the key frame over its look-ahead frames, not the raw key frame).
// A pre-processing of the SOURCE: key frame f of a chunk is replaced, in the chunk's source array, by its filter over the n frames that
// follow it (tf_rule.h: av1mi_tf_followers); everything downstream - intra coding, the motion search of frame f + 1, partition, adaptive
// quantisation, the in-loop decisions, the report's SSE - then reads the filtered frame.  Followers are read only.
//
// Two launches.  tf_search_kernel: per (16x16 block, follower, key frame) one wave runs the full search of +-R whole samples around zero
// with me_rule.h's reach, cost, index and node key - tf_search.h's body, which the temporal-dependency analysis (tpl_kernel.hip) runs
// too.  One 32-bit key per (key frame, follower, block).  tf_blend_kernel: one wave per block reads the key block into registers (4 luma + 2 chroma samples per
// lane), and per follower the displaced prediction, forms the errors' 3x3 sums through LDS and the block sums with shuffles, weighs and
// accumulates; then blends, re-extends past the signalled size and writes the block in place - blocks are disjoint, and a block reads
// the key frame inside itself only (an overhanging block's clamped coordinates stay in the block).
// Algorithmic HBM bytes per key frame with n followers: (1 + n) L b read by the search (L luma samples, b bytes each; the 2R+1-fold
// re-reads are L1 / L2 hits), (1 + n) 1.5 L b read and 1.5 L b written by the blend, 4 n L / 256 of keys each way.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "tf_rule.h"
#include "tf_search.h"

namespace {

// where the search's key of (key frame index k, follower t = 1 .. N, block b) lives
__device__ __forceinline__ size_t key_slot(int k, int N, int t, int nb, int b) { return ((size_t)k * N + (t - 1)) * nb + b; }

template <typename PIX, int R>
__global__ void __launch_bounds__(64) tf_search_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ mv, int N) {
  const int W = P.width, H = P.height, nbx = av1mi_tf_blocks(W), nb = nbx * av1mi_tf_blocks(H);
  const int b = blockIdx.x, t = blockIdx.y + 1, k = blockIdx.z, f = k * P.keyint, lane = threadIdx.x;
  uint32_t *slot = mv + key_slot(k, N, t, nb, b);
  if (t > av1mi_tf_followers(N, P.keyint, P.n_frames, f)) {   // no such follower
    if (lane == 0) *slot = AV1MI_ME_NODE_NONE;
    return;
  }
  const PIX *key = frames + (size_t)f * P.frame_samples, *ref = key + (size_t)t * P.frame_samples;   // luma of the two frames
  // (`frames` is 16-byte aligned, and the rows' strides and the frames' sizes are multiples of 8: tf_search.h loads whole words)
  uint32_t s2[8];
  const uint32_t best = tf_search_block<PIX, R>(key, ref, (b % nbx) * AV1MI_TF_BLOCK, (b / nbx) * AV1MI_TF_BLOCK, W, H, P.stride_y, lane, s2);
  if (lane == 0) *slot = best;
}

// One plane's sample of frame `fr` at clamped coordinates
template <typename PIX>
__device__ __forceinline__ int at(const PIX *__restrict__ plane, int stride, int px, int py, int w, int h) {
  return (int)plane[(size_t)tf_clampi(py, h - 1) * stride + tf_clampi(px, w - 1)];
}

template <typename PIX>
__global__ void __launch_bounds__(64) tf_blend_kernel(Av1miDevParams P, PIX *__restrict__ frames, const uint32_t *__restrict__ mv, int N, int strength) {
  // squared errors of the follower at hand - luma 16x16, then U and V 8x8 - and, at the end, the filtered block in the same layout
  __shared__ uint32_t sE[256 + 128];
  const int W = P.width, H = P.height, Wc = W >> 1, Hc = H >> 1, nbx = av1mi_tf_blocks(W), nb = nbx * av1mi_tf_blocks(H);
  const int b = blockIdx.x, k = blockIdx.y, f = k * P.keyint, lane = threadIdx.x;
  const int n = av1mi_tf_followers(N, P.keyint, P.n_frames, f);
  if (n == 0) return;   // the frame stays as it is
  const int R = P.me_range, NC = 2 * R + 1, sh = av1mi_tf_shift(strength, P.bit_depth);
  PIX *key = frames + (size_t)f * P.frame_samples;
  const int x = (b % nbx) * AV1MI_TF_BLOCK, y = (b / nbx) * AV1MI_TF_BLOCK, xc = x >> 1, yc = y >> 1;
  // this lane's samples: luma row ly, columns lx .. lx + 3; chroma plane pl (lanes 0 .. 31 U, 32 .. 63 V), row cy, columns cx, cx + 1
  const int ly = lane >> 2, lx = (lane & 3) * 4, pl = lane >> 5, cy = (lane >> 2) & 7, cx = (lane & 3) * 2;
  const long coff = pl ? P.plane_off_v : P.plane_off_u;
  int kY[4], kC[2];
  uint32_t numY[4], denY[4], numC[2], denC[2];
#pragma unroll
  for (int i = 0; i < 4; i++) { kY[i] = at(key, P.stride_y, x + lx + i, y + ly, W, H); numY[i] = 16u * (uint32_t)kY[i]; denY[i] = 16; }
#pragma unroll
  for (int i = 0; i < 2; i++) { kC[i] = at(key + coff, P.stride_c, xc + cx + i, yc + cy, Wc, Hc); numC[i] = 16u * (uint32_t)kC[i]; denC[i] = 16; }
  for (int t = 1; t <= n; t++) {
    const uint32_t idx = av1mi_me_node_index(mv[key_slot(k, N, t, nb, b)]);
    const int dy = (int)(idx / (uint32_t)NC) - R, dx = (int)(idx % (uint32_t)NC) - R;
    const PIX *ref = key + (size_t)t * P.frame_samples;
    int pY[4], pC[2];
    uint32_t bY = 0, bC = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      pY[i] = at(ref, P.stride_y, x + lx + i + dx, y + ly + dy, W, H);
      const int e = kY[i] - pY[i];
      sE[ly * 16 + lx + i] = (uint32_t)(e * e);
      bY += (uint32_t)(e * e);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int bx = av1mi_tf_chroma_base(xc + cx + i, dx), by = av1mi_tf_chroma_base(yc + cy, dy);
      const PIX *cp = ref + coff;
      pC[i] = av1mi_tf_chroma_pred(at(cp, P.stride_c, bx, by, Wc, Hc), at(cp, P.stride_c, bx + 1, by, Wc, Hc), at(cp, P.stride_c, bx, by + 1, Wc, Hc),
                                   at(cp, P.stride_c, bx + 1, by + 1, Wc, Hc), dx, dy);
      const int e = kC[i] - pC[i];
      sE[256 + pl * 64 + cy * 8 + cx + i] = (uint32_t)(e * e);
      bC += (uint32_t)(e * e);
    }
    // the block sums: luma over the wave, chroma over the plane's half of it
    for (int o = 16; o > 0; o >>= 1) { bY += __shfl_xor(bY, o, 64); bC += __shfl_xor(bC, o, 64); }
    bY += __shfl_xor(bY, 32, 64);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t S = 0;
#pragma unroll
      for (int v = -1; v <= 1; v++)
#pragma unroll
        for (int u = -1; u <= 1; u++) S += sE[tf_clampi(ly + v, 15) * 16 + tf_clampi(lx + i + u, 15)];
      const uint32_t w = (uint32_t)av1mi_tf_weight(av1mi_tf_index(S, bY, sh, 0));
      numY[i] += w * (uint32_t)pY[i]; denY[i] += w;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      uint32_t S = 0;
#pragma unroll
      for (int v = -1; v <= 1; v++)
#pragma unroll
        for (int u = -1; u <= 1; u++) S += sE[256 + pl * 64 + tf_clampi(cy + v, 7) * 8 + tf_clampi(cx + i + u, 7)];
      const uint32_t w = (uint32_t)av1mi_tf_weight(av1mi_tf_index(S, bC, sh, 1));
      numC[i] += w * (uint32_t)pC[i]; denC[i] += w;
    }
    __syncthreads();   // the next follower overwrites the errors
  }
  // the filtered block, then its samples inside the coded frame: past the signalled size the replication of the last picture column and
  // row of the FILTERED frame (they lie in this block), as the source's edge extension makes them
#pragma unroll
  for (int i = 0; i < 4; i++) sE[ly * 16 + lx + i] = (uint32_t)av1mi_tf_blend(numY[i], denY[i]);
#pragma unroll
  for (int i = 0; i < 2; i++) sE[256 + pl * 64 + cy * 8 + cx + i] = (uint32_t)av1mi_tf_blend(numC[i], denC[i]);
  __syncthreads();
  const int tw = P.true_w, th = P.true_h, twc = tw >> 1, thc = th >> 1;
  {
    const int yy = y + ly, sy = tf_clampi((yy < th ? yy : th - 1) - y, 15);
    if (yy < H) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int xx = x + lx + i, sx = tf_clampi((xx < tw ? xx : tw - 1) - x, 15);
        if (xx < W) key[(size_t)yy * P.stride_y + xx] = (PIX)sE[sy * 16 + sx];
      }
    }
  }
  {
    const int yy = yc + cy, sy = tf_clampi((yy < thc ? yy : thc - 1) - yc, 7);
    if (yy < Hc) {
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int xx = xc + cx + i, sx = tf_clampi((xx < twc ? xx : twc - 1) - xc, 7);
        if (xx < Wc) key[coff + (size_t)yy * P.stride_c + xx] = (PIX)sE[256 + pl * 64 + sy * 8 + sx];
      }
    }
  }
}

template <typename PIX>
hipError_t launch_tf(const Av1miDevParams &P, void *frames, uint32_t *mv, int N, int strength, hipStream_t stream) {
  const int nb = av1mi_tf_blocks(P.width) * av1mi_tf_blocks(P.height), nk = av1mi_tf_key_frames(P.keyint, P.n_frames);
  const dim3 gs(nb, N, nk), gb(nb, nk);
  if (P.me_range == 16) hipLaunchKernelGGL((tf_search_kernel<PIX, 16>), gs, dim3(64), 0, stream, P, (const PIX *)frames, mv, N);
  else hipLaunchKernelGGL((tf_search_kernel<PIX, 8>), gs, dim3(64), 0, stream, P, (const PIX *)frames, mv, N);
  hipLaunchKernelGGL(tf_blend_kernel<PIX>, gb, dim3(64), 0, stream, P, (PIX *)frames, (const uint32_t *)mv, N, strength);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t av1mi_launch_temporal_filter(const Av1miDevParams *P, void *frames, uint32_t *mv, int tf_frames, int tf_strength,
                                                   hipStream_t stream) {
  if (tf_frames < 1 || tf_frames > AV1MI_TF_MAX_FRAMES || tf_strength < 0 || tf_strength > AV1MI_TF_MAX_STRENGTH || (P->me_range != 8 && P->me_range != 16) ||
      P->keyint < 1 || P->n_frames < 1 || ((uintptr_t)frames & 15))
    return hipErrorInvalidValue;
  return P->bit_depth == 8 ? launch_tf<uint8_t>(*P, frames, mv, tf_frames, tf_strength, stream) : launch_tf<uint16_t>(*P, frames, mv, tf_frames, tf_strength, stream);
}
