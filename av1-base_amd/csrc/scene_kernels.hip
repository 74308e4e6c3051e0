// scene_kernels.hip - luma frame-difference statistics for the scene-cut chunker.
//
// Replaces the scene detection av1an runs before it splits a clip into chunks for its workers
// (`--workers N --temp DIR`, /root/reference/crates/daemon/src/encode/av1an.rs:100-104; SURVEY.md §8a
// row a9): SAD of the luma plane of every frame against its predecessor.  The cut rule itself is a few
// integer comparisons per frame and runs on the host (av1mi_host.cpp: decide_scene_cuts).
//
// HBM-bound streaming kernel: every luma sample of the chunk is read twice (as frame t and as frame
// t-1) with 16-byte loads per lane; algorithmic bytes 2*L*b per frame pair (L luma samples).
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "aq_rule.h"
#include "tpl_rule.h"

namespace {

__device__ __forceinline__ unsigned sad_u8x4(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

template <int BPS>
__device__ __forceinline__ unsigned sad16(const uint4 &a, const uint4 &b) {
  unsigned s = 0;
  if (BPS == 1) {
    s = sad_u8x4(a.x, b.x, s); s = sad_u8x4(a.y, b.y, s); s = sad_u8x4(a.z, b.z, s); s = sad_u8x4(a.w, b.w, s);
  } else {
    s = __builtin_amdgcn_sad_u16(a.x, b.x, s); s = __builtin_amdgcn_sad_u16(a.y, b.y, s);
    s = __builtin_amdgcn_sad_u16(a.z, b.z, s); s = __builtin_amdgcn_sad_u16(a.w, b.w, s);
  }
  return s;
}

// grid (x = slices of a frame, y = frame index t).  prev0 = predecessor of frame 0 (may be null: sad[0] = 0).
template <int BPS>
__global__ void __launch_bounds__(256) luma_sad_kernel(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ prev0,
                                                      size_t frame_bytes, size_t luma_bytes,
                                                      unsigned long long *__restrict__ sad /* [n_frames] */) {
  const int t = blockIdx.y;
  const uint8_t *cur = frames + (size_t)t * frame_bytes;
  const uint8_t *prv = t ? cur - frame_bytes : prev0;
  if (!prv) return;
  unsigned long long acc = 0;
  if (((frame_bytes | luma_bytes) & 15) == 0) {  // sizes that are multiples of 8 both ways: 16-byte loads
    const size_t nvec = luma_bytes >> 4;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(cur), *p4 = reinterpret_cast<const uint4 *>(prv);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) acc += sad16<BPS>(c4[i], p4[i]);
  } else {                                       // any other (even) size: sample by sample
    const size_t ns = luma_bytes / BPS;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (size_t)gridDim.x * 256) {
      const int a = BPS == 1 ? (int)cur[i] : (int)reinterpret_cast<const uint16_t *>(cur)[i];
      const int b = BPS == 1 ? (int)prv[i] : (int)reinterpret_cast<const uint16_t *>(prv)[i];
      acc += (unsigned long long)(a < b ? b - a : a - b);
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&sad[t], acc);
}

// ---- frame sizes that are not multiples of 8: the encoder works on frames edge-extended to the next multiple of 8.
// pad: tight planar I420 frames of w x h -> frames of cw x ch, last column / row replicated; crop: the reverse.
template <typename PIX>
__global__ void __launch_bounds__(256) pad_frames_kernel(const PIX *__restrict__ in, PIX *__restrict__ out, int w, int h, int cw, int ch) {
  const size_t in_frame = (size_t)w * h * 3 / 2, out_frame = (size_t)cw * ch * 3 / 2;
  const PIX *fi = in + (size_t)blockIdx.y * in_frame;
  PIX *fo = out + (size_t)blockIdx.y * out_frame;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < out_frame; i += (size_t)gridDim.x * 256) {
    const size_t ny = (size_t)cw * ch, nc = ny >> 2;
    const int pl = i < ny ? 0 : (i < ny + nc ? 1 : 2);
    const size_t o = i - (pl == 0 ? 0 : (pl == 1 ? ny : ny + nc));
    const int pcw = pl ? cw >> 1 : cw, pw = pl ? w >> 1 : w, ph = pl ? h >> 1 : h;
    int y = (int)(o / pcw), x = (int)(o % pcw);
    y = y < ph ? y : ph - 1; x = x < pw ? x : pw - 1;
    const size_t ioff = pl == 0 ? 0 : (pl == 1 ? (size_t)w * h : (size_t)w * h + (size_t)(w >> 1) * (h >> 1));
    fo[i] = fi[ioff + (size_t)y * pw + x];
  }
}
template <typename PIX>
__global__ void __launch_bounds__(256) crop_frames_kernel(const PIX *__restrict__ in, PIX *__restrict__ out, int w, int h, int cw, int ch) {
  const size_t in_frame = (size_t)cw * ch * 3 / 2, out_frame = (size_t)w * h * 3 / 2;
  const PIX *fi = in + (size_t)blockIdx.y * in_frame;
  PIX *fo = out + (size_t)blockIdx.y * out_frame;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < out_frame; i += (size_t)gridDim.x * 256) {
    const size_t ny = (size_t)w * h, nc = ny >> 2;
    const int pl = i < ny ? 0 : (i < ny + nc ? 1 : 2);
    const size_t o = i - (pl == 0 ? 0 : (pl == 1 ? ny : ny + nc));
    const int pw = pl ? w >> 1 : w, pcw = pl ? cw >> 1 : cw;
    const int y = (int)(o / pw), x = (int)(o % pw);
    const size_t ioff = pl == 0 ? 0 : (pl == 1 ? (size_t)cw * ch : (size_t)cw * ch + (size_t)(cw >> 1) * (ch >> 1));
    fo[i] = fi[ioff + (size_t)y * pcw + x];
  }
}

// sum and sum of squares of the 64 source luma samples of the 8x8 unit at (x0, y0), coordinates beyond the frame repeating the last
// column / row (what the block's transform will see): the statistics of the partition pass and of the activity pass
template <typename PIX>
__device__ __forceinline__ void unit_stats(const Av1miDevParams &P, const PIX *__restrict__ luma, int x0, int y0, uint32_t &S, uint32_t &Q) {
  S = 0; Q = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int yy = y0 + i < P.height ? y0 + i : P.height - 1;
    const PIX *row = luma + (size_t)yy * P.stride_y;
    if (x0 + 8 <= P.width) {   // eight samples of the row in one load (the coded width is a multiple of 8)
      if (sizeof(PIX) == 2) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + x0);
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < 4; k++) { const uint32_t a = w[k] & 0xFFFF, b = w[k] >> 16; S += a + b; Q += a * a + b * b; }
      } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(row + x0);
        const uint32_t w[2] = { v.x, v.y };
#pragma unroll
        for (int k = 0; k < 2; k++)
#pragma unroll
          for (int b8 = 0; b8 < 4; b8++) { const uint32_t a = (w[k] >> (8 * b8)) & 0xFF; S += a; Q += a * a; }
      }
    } else {
      for (int j = 0; j < 8; j++) { const int xx = x0 + j < P.width ? x0 + j : P.width - 1; const uint32_t a = row[xx]; S += a; Q += a * a; }
    }
  }
}

// ---- content-driven partition (av1mi_params.partition_search; SURVEY.md §8a row a10: the block-size decision SVT-AV1
// spends most of `--preset 3` on, /root/reference/crates/daemon/src/encode/av1an.rs:14).  Open loop, from the SOURCE luma: a node of the
// partition tree splits when its four quadrants differ in activity - the largest quadrant variance exceeds four times the smallest plus
// (ac_q / 16)^2 - so every frame of a chunk is decided in one streaming pass before any tile walk.  One wave per superblock: lane = 8x8
// unit in Z order (sum and sum of squares of its 64 samples, coordinates beyond the frame repeating the last column / row: what the
// block's transform will see), then one lane per node - sixteen 16x16, four 32x32, one 64x64 - compares its quadrants.  Writes the
// superblock's split mask (av1mi_dev.h: av1mi_node_split reads it).  Algorithmic bytes L b per frame (L luma samples).
template <typename PIX>
__global__ void __launch_bounds__(64) partition_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint32_t *__restrict__ part) {
  __shared__ uint32_t uS[64], uQ[64];
  __shared__ uint32_t bits[21];
  const int f = blockIdx.y, sb = blockIdx.x, lane = threadIdx.x;
  const int sb_x = (sb % P.sb_cols) * 64, sb_y = (sb / P.sb_cols) * 64;
  const PIX *luma = frames + (size_t)f * P.frame_samples;
  {
    const int ux = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4), uy = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
    uint32_t S, Q;
    unit_stats(P, luma, sb_x + 8 * ux, sb_y + 8 * uy, S, Q);
    uS[lane] = S; uQ[lane] = Q;
  }
  __syncthreads();
  if (lane < 21) {
    // node of this lane: 0 .. 15 the 16x16 nodes (Z order; quadrants = 1 unit each), 16 .. 19 the 32x32 nodes (4 units per quadrant), 20 the
    // 64x64 node (16 units per quadrant); the units of a node are consecutive in Z order
    const int per_q = lane < 16 ? 1 : (lane < 20 ? 4 : 16);
    const int first = lane < 16 ? 4 * lane : (lane < 20 ? 16 * (lane - 16) : 0);
    const unsigned long long m = 64ull * per_q, t = (unsigned long long)(P.ac_q >> 4);
    unsigned long long vmin = ~0ull, vmax = 0;
    for (int q = 0; q < 4; q++) {
      unsigned long long S = 0, Q = 0;
      for (int u = 0; u < per_q; u++) { S += uS[first + q * per_q + u]; Q += uQ[first + q * per_q + u]; }
      const unsigned long long V = m * Q - S * S;
      vmin = V < vmin ? V : vmin;
      vmax = V > vmax ? V : vmax;
    }
    // bit 0: the 64x64 node, bits 1 .. 4: the 32x32 nodes, bits 5 .. 20: the 16x16 nodes
    bits[lane < 16 ? 5 + lane : (lane < 20 ? 1 + (lane - 16) : 0)] = vmax > 4 * vmin + t * t * m * m;
  }
  __syncthreads();
  if (lane == 0) {
    uint32_t mask = 0;
    for (int b = 0; b < 21; b++) mask |= (bits[b] & 1u) << b;
    part[(size_t)f * P.sb_rows * P.sb_cols + sb] = mask;
  }
}

// ---- activity-adaptive quantisation (av1mi_params.cq_level bits 8-10; aq_rule.h is the rule).  Open loop, from
// the SOURCE luma, for all frames of a chunk before any tile walk.  First launch: one wave per superblock, lane = 8x8 unit (the
// partition pass's statistics), e per unit, E = the rounded mean over the units inside the coded frame -> act[frame][superblock].
// Second launch: one workgroup per frame sums E (integers: any order gives the same M) and writes the superblocks' quantiser indices.
// Algorithmic bytes L b per frame (L luma samples) + 3 per superblock.
template <typename PIX>
__global__ void __launch_bounds__(64) aq_activity_kernel(Av1miDevParams P, const PIX *__restrict__ frames, uint16_t *__restrict__ act) {
  const int f = blockIdx.y, sb = blockIdx.x, lane = threadIdx.x;
  const int x0 = (sb % P.sb_cols) * 64 + 8 * (lane & 7), y0 = (sb / P.sb_cols) * 64 + 8 * (lane >> 3);
  const bool inside = x0 < P.width && y0 < P.height;
  uint32_t e = 0;
  if (inside) {
    uint32_t S, Q;
    unit_stats(P, frames + (size_t)f * P.frame_samples, x0, y0, S, Q);
    e = (uint32_t)av1mi_aq_unit_energy(S, Q, P.bit_depth);
  }
  uint32_t n = inside ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o, 64); n += __shfl_xor(n, o, 64); }
  if (lane == 0) act[(size_t)f * P.sb_rows * P.sb_cols + sb] = (uint16_t)av1mi_aq_mean(e, n);
}

// beta, beta_sum, tpl_strength: the temporal term (tpl_rule.h) - beta per [frame][superblock] and the chunk's sum of it, from
// av1mi_launch_tpl on the same stream before; strength 0: neither is read and the map is the spatial rule's.  A spatial strength of 0
// does not read act.
// F: the frame term (tpl_rule.h "frame"), F.strength 0 = off.  On: the workgroup forms MF from the chunk's n values of betaF
// (tpl_frame_kernel on the same stream before), then its frame's k_f and q_f - into F.fq.frame_q and into the eight bits of base_q_idx
// in the frame's header slot - and writes the map q_f + 4 d, the temporal term against the frame's own mean and the clamp against q_f;
// all q_f when both superblock strengths are 0.
__global__ void __launch_bounds__(256) aq_map_kernel(Av1miDevParams P, const uint16_t *__restrict__ act, uint8_t *__restrict__ qmap, int strength,
                                                     const uint16_t *__restrict__ beta, const unsigned long long *__restrict__ beta_sum, int tpl_strength,
                                                     Av1miFqMap F) {
  __shared__ uint32_t part[4], fpart[4];
  const int f = blockIdx.x, t = threadIdx.x, nsb = P.sb_rows * P.sb_cols;
  const uint16_t *E = act + (size_t)f * nsb;
  uint32_t sum = 0;
  if (strength) for (int i = t; i < nsb; i += 256) sum += E[i];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((t & 63) == 0) part[t >> 6] = sum;
  __syncthreads();
  const int M = av1mi_aq_mean(part[0] + part[1] + part[2] + part[3], (uint32_t)nsb);
  if (F.strength) {
    uint32_t bf = 0;
    for (int i = t; i < P.n_frames; i += 256) bf += F.fq.beta[i];
    for (int o = 32; o > 0; o >>= 1) bf += __shfl_xor(bf, o, 64);
    if ((t & 63) == 0) fpart[t >> 6] = bf;
    __syncthreads();
    const int MF = av1mi_fq_mean((uint64_t)fpart[0] + fpart[1] + fpart[2] + fpart[3], (uint64_t)P.n_frames);
    const int qf = av1mi_fq_qindex(F.strength, (int)F.fq.beta[f], MF, P.base_q_idx);
    const int Mbf = tpl_strength ? av1mi_tpl_mean_beta(F.fq.sb_beta_sum[f], (uint64_t)nsb) : 0;
    for (int i = t; i < nsb; i += 256)
      qmap[(size_t)f * nsb + i] = (uint8_t)(strength || tpl_strength ? av1mi_fq_sb_qindex(strength, strength ? (int)E[i] : 0, M, tpl_strength,
                                                                                        tpl_strength ? (int)beta[(size_t)f * nsb + i] : 0, Mbf, qf)
                                                                    : qf);
    if (t == 0) {
      F.fq.frame_q[f] = (uint8_t)qf;
      if (F.hdr_blob) {
        uint8_t *h = F.hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
        int bit = F.q_bit[av1mi_frame_is_inter(P, f)];
        for (int k = 7; k >= 0; k--, bit++) {
          const uint8_t m = (uint8_t)(0x80 >> (bit & 7));
          h[bit >> 3] = ((qf >> k) & 1) ? (uint8_t)(h[bit >> 3] | m) : (uint8_t)(h[bit >> 3] & ~m);
        }
      }
    }
    return;
  }
  if (!tpl_strength) {
    for (int i = t; i < nsb; i += 256) qmap[(size_t)f * nsb + i] = (uint8_t)av1mi_aq_qindex_of(strength, (int)E[i], M, P.base_q_idx);
    return;
  }
  const int Mb = av1mi_tpl_mean_beta(*beta_sum, (uint64_t)P.n_frames * (uint64_t)nsb);
  for (int i = t; i < nsb; i += 256)
    qmap[(size_t)f * nsb + i] = (uint8_t)av1mi_tpl_qindex_of(strength, strength ? (int)E[i] : 0, M, tpl_strength, (int)beta[(size_t)f * nsb + i], Mb, P.base_q_idx);
}

}  // namespace

extern "C" hipError_t av1mi_launch_partition(const Av1miDevParams *P, const void *frames, uint32_t *part, hipStream_t stream) {
  dim3 grid(P->sb_rows * P->sb_cols, P->n_frames);
  if (P->bit_depth == 8) hipLaunchKernelGGL(partition_kernel<uint8_t>, grid, dim3(64), 0, stream, *P, (const uint8_t *)frames, part);
  else hipLaunchKernelGGL(partition_kernel<uint16_t>, grid, dim3(64), 0, stream, *P, (const uint16_t *)frames, part);
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_aq(const Av1miDevParams *P, const void *frames, uint16_t *act, uint8_t *qmap, int strength, const uint16_t *beta,
                                      const unsigned long long *beta_sum, int tpl_strength, const Av1miFqMap *fq, hipStream_t stream) {
  Av1miFqMap F = {};
  if (fq && fq->strength) {
    if (!fq->fq.beta || !fq->fq.sb_beta_sum || !fq->fq.frame_q) return hipErrorInvalidValue;
    F = *fq;
  }
  dim3 grid(P->sb_rows * P->sb_cols, P->n_frames);
  if (!strength) { }   // the spatial term is 0: no activity pass
  else if (P->bit_depth == 8) hipLaunchKernelGGL(aq_activity_kernel<uint8_t>, grid, dim3(64), 0, stream, *P, (const uint8_t *)frames, act);
  else hipLaunchKernelGGL(aq_activity_kernel<uint16_t>, grid, dim3(64), 0, stream, *P, (const uint16_t *)frames, act);
  hipLaunchKernelGGL(aq_map_kernel, dim3(P->n_frames), dim3(256), 0, stream, *P, (const uint16_t *)act, qmap, strength, beta, beta_sum, tpl_strength, F);
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_pad(const void *in, void *out, int w, int h, int cw, int ch, int bit_depth, int n_frames, int crop,
                                       hipStream_t stream) {
  dim3 grid(256, n_frames);
  if (bit_depth == 8) {
    if (crop) hipLaunchKernelGGL(crop_frames_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t *)in, (uint8_t *)out, w, h, cw, ch);
    else hipLaunchKernelGGL(pad_frames_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t *)in, (uint8_t *)out, w, h, cw, ch);
  } else {
    if (crop) hipLaunchKernelGGL(crop_frames_kernel<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t *)in, (uint16_t *)out, w, h, cw, ch);
    else hipLaunchKernelGGL(pad_frames_kernel<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t *)in, (uint16_t *)out, w, h, cw, ch);
  }
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_luma_sad(const Av1miDevParams *P, const void *frames, const void *prev0, unsigned long long *sad,
                                            hipStream_t stream) {
  const int bps = P->bit_depth > 8 ? 2 : 1;
  const size_t frame_bytes = (size_t)P->frame_samples * bps, luma_bytes = (size_t)P->width * P->height * bps;
  dim3 grid(128, P->n_frames);
  if (bps == 1)
    hipLaunchKernelGGL(luma_sad_kernel<1>, grid, dim3(256), 0, stream, (const uint8_t *)frames, (const uint8_t *)prev0, frame_bytes, luma_bytes, sad);
  else
    hipLaunchKernelGGL(luma_sad_kernel<2>, grid, dim3(256), 0, stream, (const uint8_t *)frames, (const uint8_t *)prev0, frame_bytes, luma_bytes, sad);
  return hipGetLastError();
}
