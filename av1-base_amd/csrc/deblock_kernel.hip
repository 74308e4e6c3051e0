// deblock_kernel.hip - AV1 deblocking filter (spec §7.14), in place on the reconstruction before
// CDEF.  Replaces the loop-filter stage of the SVT-AV1 worker behind `run_av1an`
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139).  Restated in oracle/av1o_deblock.c (pinned by dav1d).
//
// Structure of this build: square blocks, transform == block, no segmentation or loop-filter deltas - every transform
// edge is a block edge and the level is frame-wide.  Per plane all vertical edges are filtered, then all horizontal
// edges; within one pass the edges are independent (a filter modifies at most 6 samples and reads at most 7 on each
// side, and reaches that far only when both neighbouring transforms are >= 16 wide), so one pass is one launch:
// one thread per 4-sample edge segment of any plane.  HBM bound: each pass reads and writes the samples next to the
// edges; algorithmic bytes <= 2 * 2 * N * b per frame (both passes, read + write).
// The level is the quantiser's (deblock = 1) or, per frame and plane, the one deblock_search_kernel + deblock_decide_kernel below chose
// by squared error against the source (deblock = 2); filter, edge predicate and limits are deblock_pieces.h's for all of them.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "deblock_pieces.h"

namespace {

// PASS 0: vertical edges, 1: horizontal edges.  grid.x covers the 4x4 positions of all three planes, grid.y = frame.
// lf_sel: null - the levels of the parameter block; else the level search's four levels per frame of the launch
template <typename PIX, int PASS>
__global__ void __launch_bounds__(256) deblock_kernel(Av1miDevParams P, PIX *__restrict__ rec, const Av1miBlkInfo *__restrict__ blk,
                                                     const uint8_t *__restrict__ lf_sel) {
  const int f = blockIdx.y;
  const long n_luma = (long)P.mi_rows * P.mi_cols, n_chroma = n_luma >> 2;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n_luma + 2 * n_chroma) return;
  const int plane = id < n_luma ? 0 : (id < n_luma + n_chroma ? 1 : 2);
  const long local = id - (plane == 0 ? 0 : (plane == 1 ? n_luma : n_luma + n_chroma));
  const int ss = plane > 0;
  const int pcols = P.mi_cols >> ss;
  const int r4 = (int)(local / pcols), c4 = (int)(local % pcols);   // 4x4 position in the plane
  const int li = plane == 0 ? PASS : plane + 1;
  const int lvl = lf_sel ? (int)lf_sel[f * 4 + li] : P.lf_level[li];
  if (!lvl) return;
  const Av1miBlkInfo *info = blk + (size_t)f * P.b8_rows * P.b8_cols;
  const int len = av1mi_lf_edge_len(plane, PASS, r4, c4, info, P.b8_cols, P.true_w, P.true_h);
  if (!len) return;
  int lim, blim, thr;
  av1mi_lf_limits(lvl, P.lf_sharpness, P.bit_depth, &lim, &blim, &thr);
  const int x = c4 * 4, y = r4 * 4;
  const long stride = plane ? P.stride_c : P.stride_y;
  PIX *pl = rec + (size_t)f * P.frame_samples + (plane == 0 ? 0 : (plane == 1 ? P.plane_off_u : P.plane_off_v));
#pragma unroll
  for (int i = 0; i < 4; i++) {
    PIX *px = pl + (size_t)(y + (PASS ? 0 : i)) * stride + x + (PASS ? i : 0);
    av1mi_lf_filter_sample<PIX, long>(px, PASS ? stride : 1, plane, lim, blim, thr, len, P.bit_depth);
  }
}

// ---- the level search (av1mi_params.deblock = 2).  One workgroup per (frame, plane, 64x64 superblock):
// blockIdx.x < sb_rows * sb_cols - luma, then U, then V; blockIdx.y - frame frame0 + y of the chunk.  The superblock's tile of the
// frame's reconstruction before deblocking (deblock_pieces.h: interior + halo, positions outside the plane clamped) goes into LDS once;
// per candidate level the working copy is restored, filtered - vertical pass on every tile row, then horizontal pass on the interior's
// columns, the lines of a pass spread over the lanes - and the interior's squared error against the source, within the signalled size,
// is summed: 32 bits per lane (16 samples of at most 1023^2), 64 across the workgroup, one atomicAdd per candidate into
// lf_err[frame][plane][candidate].  Levels, limits and loop bounds are wave-uniform.  Neighbouring candidates that clamp to the same
// level are filtered once.
template <typename PIX>
__global__ void __launch_bounds__(256) deblock_search_kernel(Av1miDevParams P, int frame0, const PIX *__restrict__ rec, const PIX *__restrict__ src,
                                                            const Av1miBlkInfo *__restrict__ blk) {
  __shared__ __attribute__((aligned(16))) uint16_t pristine[AV1MI_LF_TILE_SAMPLES], work[AV1MI_LF_TILE_SAMPLES];
  __shared__ uint8_t seg[2][AV1MI_LF_EDGES][AV1MI_LF_SEGS];
  __shared__ unsigned long long wave_sum[4];
  const int t = threadIdx.x, f = frame0 + (int)blockIdx.y;
  const int nsb = P.sb_rows * P.sb_cols;
  const int plane = (int)blockIdx.x / nsb, sb = (int)blockIdx.x % nsb;
  const Av1miLfTile T = av1mi_lf_tile(plane, sb / P.sb_cols, sb % P.sb_cols, P.width, P.height);
  const long stride = plane ? P.stride_c : P.stride_y;
  const size_t plane_off = (size_t)f * P.frame_samples + (plane == 0 ? 0 : (plane == 1 ? P.plane_off_u : P.plane_off_v));
  const PIX *rp = rec + plane_off, *sp = src + plane_off;
  const Av1miBlkInfo *info = blk + (size_t)f * P.b8_rows * P.b8_cols;
  for (int i = t; i < T.T * T.T; i += 256) {
    int py, px;
    av1mi_lf_tile_source(T, i / T.T, i % T.T, &py, &px);
    pristine[(i / T.T) * AV1MI_LF_PITCH + i % T.T] = (uint16_t)rp[(size_t)py * stride + px];
  }
  for (int i = t; i < 2 * AV1MI_LF_EDGES * AV1MI_LF_SEGS; i += 256) {
    const int pass = i / (AV1MI_LF_EDGES * AV1MI_LF_SEGS), e = i / AV1MI_LF_SEGS % AV1MI_LF_EDGES, k = i % AV1MI_LF_SEGS;
    seg[pass][e][k] = k * 4 < (pass ? T.S : T.T) ? (uint8_t)av1mi_lf_tile_seg_len(T, pass, e, k, info, P.b8_cols, P.true_w, P.true_h) : 0;
  }
  // this lane's interior samples: sample i = k * 256 + t, row i / S; the source where the sample counts, -1 where it lies beyond the signalled size
  const int per_lane = T.S * T.S / 256;   // 16 / 4
  const int tw = plane ? (P.true_w + 1) >> 1 : P.true_w, th = plane ? (P.true_h + 1) >> 1 : P.true_h;
  int want[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    if (k >= per_lane) break;   // (wave-uniform: a chroma item has 4 samples per lane)
    const int i = k * 256 + t, iy = i / T.S, ix = i % T.S;
    want[k] = (T.x0 + ix < tw && T.y0 + iy < th) ? (int)sp[(size_t)(T.y0 + iy) * stride + T.x0 + ix] : -1;
  }
  const int g = P.lf_search_g[av1mi_frame_is_inter(P, f)];
  unsigned long long *err = P.lf_err + ((size_t)f * 3 + plane) * AV1MI_LF_CANDS;
  unsigned long long total = 0;   // (thread 0) the last filtered candidate's sum
  int last = -1;
  const int n0 = av1mi_lf_tile_lines(T, 0), n1 = av1mi_lf_tile_lines(T, 1);
  for (int c = 0; c < AV1MI_LF_CANDS; c++) {
    const int lvl = av1mi_lf_pool(g, c, plane > 0);
    if (lvl != last) {
      last = lvl;
      __syncthreads();   // the tile and the tables are written / the error pass before has read the working copy
      // whole rows, 32 bits at a time: the two pad columns behind each row come along, never written and never read
      for (int i = t; i < T.T * AV1MI_LF_PITCH / 2; i += 256) ((uint32_t *)work)[i] = ((const uint32_t *)pristine)[i];
      __syncthreads();
      if (lvl) {
        int lim, blim, thr;
        av1mi_lf_limits(lvl, P.lf_sharpness, P.bit_depth, &lim, &blim, &thr);
        for (int L = t; L < n0; L += 256) {
          int e, k;
          const int off = av1mi_lf_tile_line(T, 0, L, &e, &k), len = seg[0][e][k];
          if (len) av1mi_lf_filter_sample<uint16_t, int>(work + off, 1, plane, lim, blim, thr, len, P.bit_depth);
        }
        __syncthreads();
        for (int L = t; L < n1; L += 256) {
          int e, k;
          const int off = av1mi_lf_tile_line(T, 1, L, &e, &k), len = seg[1][e][k];
          if (len) av1mi_lf_filter_sample<uint16_t, int>(work + off, AV1MI_LF_PITCH, plane, lim, blim, thr, len, P.bit_depth);
        }
        __syncthreads();
      }
      uint32_t acc = 0;
#pragma unroll
      for (int k = 0; k < 16; k++) {
        if (k >= per_lane) break;
        const int i = k * 256 + t, iy = i / T.S, ix = i % T.S;
        if (want[k] >= 0) { const int d = (int)work[(T.H + iy) * AV1MI_LF_PITCH + T.H + ix] - want[k]; acc += (uint32_t)(d * d); }
      }
      unsigned long long v = acc;
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((t & 63) == 0) wave_sum[t >> 6] = v;
      __syncthreads();
      if (t == 0) total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    }
    if (t == 0 && total) atomicAdd(err + c, total);
  }
}

// The frame's levels from its error table (one workgroup per frame of the launch): per plane the first minimum, into lf_sel[frame][4] -
// luma's level for both of its passes - and into the 24 bits of loop_filter_level[0..3] in the frame's header slot, where the host wrote
// placeholders (lf_bit[key / inter]).
__global__ void __launch_bounds__(64) deblock_decide_kernel(Av1miDevParams P, int frame0, uint8_t *__restrict__ hdr_blob) {
  __shared__ int lv[3];
  const int f = frame0 + (int)blockIdx.x, t = threadIdx.x;
  const int inter = av1mi_frame_is_inter(P, f);
  if (t < 3) lv[t] = av1mi_lf_pool(P.lf_search_g[inter], av1mi_lf_first_min(P.lf_err + ((size_t)f * 3 + t) * AV1MI_LF_CANDS), t > 0);
  __syncthreads();
  if (t < 4) P.lf_sel[f * 4 + t] = (uint8_t)lv[t < 2 ? 0 : t - 1];
  if (t == 0) {
    uint8_t *h = hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
    int bit = P.lf_bit[inter];
    const uint32_t v = ((uint32_t)lv[0] << 18) | ((uint32_t)lv[0] << 12) | ((uint32_t)lv[1] << 6) | (uint32_t)lv[2];
    for (int k = 23; k >= 0; k--, bit++) {
      const uint8_t m = (uint8_t)(0x80 >> (bit & 7));
      h[bit >> 3] = ((v >> k) & 1) ? (uint8_t)(h[bit >> 3] | m) : (uint8_t)(h[bit >> 3] & ~m);
    }
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_deblock(const Av1miDevParams *P, void *rec, const Av1miBlkInfo *blk, int frame0, int count, hipStream_t stream) {
  Av1miDevParams R = av1mi_frame_range(*P, frame0, count);
  for (int i = 0; i < 4; i++) R.lf_level[i] = av1mi_frame_lf_levels(*P, frame0)[i];
  rec = av1mi_frame_at(R, rec, frame0); blk += (size_t)frame0 * R.b8_rows * R.b8_cols;
  const long n = (long)R.mi_rows * R.mi_cols * 3 / 2;
  dim3 grid((unsigned)((n + 255) / 256), count);
  const uint8_t *sel = R.lf_search ? R.lf_sel : nullptr;
  if (R.bit_depth == 8) {
    hipLaunchKernelGGL((deblock_kernel<uint8_t, 0>), grid, dim3(256), 0, stream, R, (uint8_t *)rec, blk, sel);
    hipLaunchKernelGGL((deblock_kernel<uint8_t, 1>), grid, dim3(256), 0, stream, R, (uint8_t *)rec, blk, sel);
  } else {
    hipLaunchKernelGGL((deblock_kernel<uint16_t, 0>), grid, dim3(256), 0, stream, R, (uint16_t *)rec, blk, sel);
    hipLaunchKernelGGL((deblock_kernel<uint16_t, 1>), grid, dim3(256), 0, stream, R, (uint16_t *)rec, blk, sel);
  }
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_deblock_search(const Av1miDevParams *P, const void *rec, const void *src, const Av1miBlkInfo *blk, uint8_t *hdr_blob,
                                                  int frame0, int count, hipStream_t stream) {
  if (!P->lf_search || !P->lf_err || !P->lf_sel) return hipErrorInvalidValue;
  dim3 grid((unsigned)(3 * P->sb_rows * P->sb_cols), count);
  if (P->bit_depth == 8) hipLaunchKernelGGL((deblock_search_kernel<uint8_t>), grid, dim3(256), 0, stream, *P, frame0, (const uint8_t *)rec, (const uint8_t *)src, blk);
  else hipLaunchKernelGGL((deblock_search_kernel<uint16_t>), grid, dim3(256), 0, stream, *P, frame0, (const uint16_t *)rec, (const uint16_t *)src, blk);
  hipLaunchKernelGGL(deblock_decide_kernel, dim3(count), dim3(64), 0, stream, *P, frame0, hdr_blob);
  return hipGetLastError();
}
