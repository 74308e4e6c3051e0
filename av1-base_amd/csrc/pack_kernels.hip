// pack_kernels.hip - bitstream packing, and the squared error (PSNR) of the reconstruction.
//
// The packing replaces av1an's chunk concatenation (`-o`, av1an.rs:87) at tile
// granularity: prefix sums over tile sizes, then every tile copies itself into the final
// Section-5 OBU stream (temporal delimiter, sequence header, OBU_FRAME with tile sizes).
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"

namespace {

// ------------------------------------------------------------------------------ SSE (PSNR)
// 16 bytes per lane per load (8 or 16 samples); plane sizes are multiples of 16 samples (width, height multiples of 8),
// so a vector never straddles two planes.  VEC = false: sample-wise fallback for frame pointers that are not 16-byte aligned.
template <typename PIX, bool VEC>
__global__ void __launch_bounds__(256) sse_kernel(Av1miDevParams P, const PIX *__restrict__ a, const PIX *__restrict__ b,
                                                 unsigned long long *__restrict__ sse /* [n_frames][3] */) {
  const int f = blockIdx.y;
  const PIX *pa = a + (size_t)f * P.frame_samples, *pb = b + (size_t)f * P.frame_samples;
  const long ny = (long)P.width * P.height, nc = ny >> 2;
  unsigned long long acc[3] = { 0, 0, 0 };
  if (VEC) {
    constexpr int SPV = 16 / (int)sizeof(PIX);  // samples per vector
    const uint4 *va = reinterpret_cast<const uint4 *>(pa), *vb = reinterpret_cast<const uint4 *>(pb);
    const long nvec = P.frame_samples / SPV;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
      const uint4 x = va[i], y = vb[i];
      const uint32_t xs[4] = { x.x, x.y, x.z, x.w }, ys[4] = { y.x, y.y, y.z, y.w };
      unsigned s = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (sizeof(PIX) == 2) {
          const int d0 = (int)(xs[k] & 0xFFFF) - (int)(ys[k] & 0xFFFF), d1 = (int)(xs[k] >> 16) - (int)(ys[k] >> 16);
          s += (unsigned)(d0 * d0) + (unsigned)(d1 * d1);
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++) { const int d = (int)((xs[k] >> (8 * q)) & 0xFF) - (int)((ys[k] >> (8 * q)) & 0xFF); s += (unsigned)(d * d); }
        }
      }
      const long i0 = i * SPV;
      const int pl = i0 < ny ? 0 : (i0 < ny + nc ? 1 : 2);
      acc[pl] += s;
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P.frame_samples; i += (long)gridDim.x * 256) {
      const int d = (int)pa[i] - (int)pb[i];
      const int pl = i < ny ? 0 : (i < ny + nc ? 1 : 2);
      acc[pl] += (unsigned long long)(d * d);
    }
  }
  for (int pl = 0; pl < 3; pl++) {
    unsigned long long v = acc[pl];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sse[f * 3 + pl], v);
  }
}

// ------------------------------------------------------------------------------ packing
__device__ __forceinline__ int leb128_len(uint32_t v) {
  int n = 1;
  while (v >>= 7) n++;
  return n;
}

// one workgroup per frame: tile offsets inside the OBU_FRAME payload, frame (temporal unit) size; with a chunk record (P.chunk_record)
// the frame's tiles' symbol counts go into it (integer sum and maximum: the order of the frames' additions does not show)
__global__ void __launch_bounds__(256) frame_layout_kernel(Av1miDevParams P, const uint32_t *__restrict__ tile_bytes,
                                                          uint32_t *__restrict__ tile_off, uint32_t *__restrict__ frame_size,
                                                          uint32_t *__restrict__ payload_size, int *__restrict__ overflow) {
  __shared__ uint32_t part[256];
  __shared__ unsigned long long sym_sum[256];
  __shared__ uint32_t sym_max[256];
  const int f = blockIdx.x, nt = P.tile_rows * P.tile_cols, t = threadIdx.x;
  const uint32_t *tb = tile_bytes + (size_t)f * nt;
  const int per = (nt + 255) / 256;
  uint32_t s = 0;
  if (P.chunk_record) {
    const uint32_t *sl = P.tile_symbols + (size_t)f * nt;
    unsigned long long ssum = 0;
    uint32_t smax = 0;
    for (int i = t * per; i < (t + 1) * per && i < nt; i++) { ssum += sl[i]; smax = sl[i] > smax ? sl[i] : smax; }
    sym_sum[t] = ssum; sym_max[t] = smax;
  }
  for (int i = t * per; i < (t + 1) * per && i < nt; i++) {
    // a tile that outgrew its slot or its symbol stream (0xFFFFFFFF): flag it; the host re-runs the
    // chunk with larger capacities and pack_tiles_kernel does nothing in this pass
    if (tb[i] > (uint32_t)P.tile_slot_bytes) atomicExch(overflow, 1);
    s += tb[i] + (i < nt - 1 ? (uint32_t)P.tile_size_bytes : 0u);
  }
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    // temporal unit = TD + [sequence header, key frames only] + OBU_FRAME header + size + payload
    const int inter = av1mi_frame_is_inter(P, f);
    uint32_t run = (uint32_t)(inter ? P.inter_hdr_bytes : P.frame_hdr_bytes);
    for (int i = 0; i < 256; i++) { uint32_t v = part[i]; part[i] = run; run += v; }
    payload_size[f] = run;
    frame_size[f] = 2u + (inter ? 0u : (uint32_t)P.seq_hdr_bytes) + 1u + (uint32_t)leb128_len(run) + run;
    if (P.chunk_record) {
      unsigned long long ssum = 0;
      uint32_t smax = 0;
      for (int i = 0; i < 256; i++) { ssum += sym_sum[i]; smax = sym_max[i] > smax ? sym_max[i] : smax; }
      atomicAdd(&P.chunk_record->n_symbols, ssum);
      atomicMax(&P.chunk_record->max_tile_symbols, smax);
    }
  }
  __syncthreads();
  uint32_t run = part[t];
  for (int i = t * per; i < (t + 1) * per && i < nt; i++) {
    tile_off[(size_t)f * nt + i] = run;
    run += tb[i] + (i < nt - 1 ? (uint32_t)P.tile_size_bytes : 0u);
  }
}

__global__ void chunk_layout_kernel(int n_frames, const uint32_t *__restrict__ frame_size, unsigned long long *__restrict__ frame_off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    unsigned long long run = 0;
    for (int f = 0; f < n_frames; f++) { frame_off[f] = run; run += frame_size[f]; }
    frame_off[n_frames] = run;
  }
}

// one wave per tile: copy the tile (and, for tile 0, the frame's headers) to its final position
__global__ void __launch_bounds__(64) pack_tiles_kernel(Av1miDevParams P, const uint8_t *__restrict__ slots,
                                                       const uint32_t *__restrict__ tile_bytes, const uint32_t *__restrict__ tile_off,
                                                       const uint32_t *__restrict__ payload_size,
                                                       const unsigned long long *__restrict__ frame_off,
                                                       const uint8_t *__restrict__ hdr_blob, uint8_t *__restrict__ out,
                                                       const int *__restrict__ overflow) {
  if (*overflow) return;  // sizes and offsets are meaningless: nothing may be written
  const int nt = P.tile_rows * P.tile_cols;
  const int f = blockIdx.x / nt, t = blockIdx.x % nt, lane = threadIdx.x;
  const uint32_t pay = payload_size[f];
  const int ll = leb128_len(pay);
  uint8_t *fo = out + frame_off[f];
  const int inter = av1mi_frame_is_inter(P, f);
  const int seq_bytes = inter ? 0 : P.seq_hdr_bytes, hdr_bytes = inter ? P.inter_hdr_bytes : P.frame_hdr_bytes;
  const int prefix = 2 + seq_bytes + 1 + ll;  // TD + [sequence header] + OBU_FRAME header + size
  if (t == 0) {
    if (lane == 0) {
      fo[0] = 0x12; fo[1] = 0x00;
      uint8_t *q = fo + 2 + seq_bytes;
      q[0] = 0x32;
      uint32_t v = pay;
      for (int i = 0; i < ll; i++) { uint8_t b = v & 0x7F; v >>= 7; if (v) b |= 0x80; q[1 + i] = b; }
    }
    for (int i = lane; i < seq_bytes; i += 64) fo[2 + i] = hdr_blob[i];
    for (int i = lane; i < hdr_bytes; i += 64) fo[prefix + i] = hdr_blob[P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes + i];
  }
  const uint32_t n = tile_bytes[blockIdx.x];
  uint8_t *dst = fo + prefix + tile_off[blockIdx.x];
  if (t < nt - 1) {
    if (lane < P.tile_size_bytes) dst[lane] = (uint8_t)((n - 1) >> (8 * lane));
    dst += P.tile_size_bytes;
  }
  // The range-coding kernel left 16-bit pre-carry entries d[i] = byte | carry << 8 (carry: +1 to the number formed by the
  // bytes before i).  Final byte i = (lo(d[i]) + hi(d[i+1]) + carry-in from the right) & 0xFF: a long addition whose
  // carries are resolved 64 positions at a time, from the end of the tile, with generate/propagate masks and one 64-bit
  // add per chunk (carry-lookahead: carries = (X + Y + cin) ^ P with X = G | P, Y = G).
  const uint16_t *pre = reinterpret_cast<const uint16_t *>(slots) + (size_t)blockIdx.x * P.tile_slot_bytes;
  unsigned long long carry = 0;
  for (long base = n ? (long)((n - 1) & ~63u) : -1; base >= 0; base -= 64) {
    const uint32_t i = (uint32_t)base + (uint32_t)lane;
    const bool valid = i < n;
    const unsigned d = valid ? pre[i] : 0u, dn = (i + 1 < n) ? pre[i + 1] : 0u;
    const unsigned sv = (d & 0xFFu) + (dn >> 8);                 // 0 .. 256
    // bit (63 - lane): carries run from larger i (low bits) to smaller i (high bits)
    const unsigned long long G = __brevll(__ballot(valid && sv == 256u)), Pm = __brevll(__ballot(valid && sv == 255u));
    const unsigned long long X = G | Pm;
    const unsigned long long S1 = X + G, S = S1 + carry;
    const unsigned long long cout = (S1 < X) | (S < S1);         // carry out of bit 63 = into the previous chunk
    const unsigned long long C = S ^ Pm;                         // S ^ X ^ Y: carry into every position
    const unsigned cin = (unsigned)((C >> (63 - lane)) & 1ull);
    if (valid) dst[i] = (uint8_t)(sv + cin);
    carry = cout;
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_sse(const Av1miDevParams *P, const void *a, const void *b, unsigned long long *sse, hipStream_t stream) {
  dim3 grid(64, P->n_frames);
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;  // frame size in bytes is a multiple of 16 (1.5 * w * h, w and h multiples of 8)
  if (P->bit_depth == 8) {
    if (vec) hipLaunchKernelGGL((sse_kernel<uint8_t, true>), grid, dim3(256), 0, stream, *P, (const uint8_t *)a, (const uint8_t *)b, sse);
    else hipLaunchKernelGGL((sse_kernel<uint8_t, false>), grid, dim3(256), 0, stream, *P, (const uint8_t *)a, (const uint8_t *)b, sse);
  } else {
    if (vec) hipLaunchKernelGGL((sse_kernel<uint16_t, true>), grid, dim3(256), 0, stream, *P, (const uint16_t *)a, (const uint16_t *)b, sse);
    else hipLaunchKernelGGL((sse_kernel<uint16_t, false>), grid, dim3(256), 0, stream, *P, (const uint16_t *)a, (const uint16_t *)b, sse);
  }
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_pack(const Av1miDevParams *P, const uint8_t *slots, const uint32_t *tile_bytes, uint32_t *tile_off,
                                        uint32_t *frame_size, uint32_t *payload_size, unsigned long long *frame_off,
                                        const uint8_t *hdr_blob, uint8_t *out, int *overflow, int stage, hipStream_t stream) {
  const int nt = P->tile_rows * P->tile_cols;
  if (stage == 0) {
    hipLaunchKernelGGL(frame_layout_kernel, dim3(P->n_frames), dim3(256), 0, stream, *P, tile_bytes, tile_off, frame_size, payload_size, overflow);
    hipLaunchKernelGGL(chunk_layout_kernel, dim3(1), dim3(64), 0, stream, P->n_frames, frame_size, frame_off);
  } else {
    hipLaunchKernelGGL(pack_tiles_kernel, dim3(P->n_frames * nt), dim3(64), 0, stream, *P, slots, tile_bytes, tile_off, payload_size, frame_off, hdr_blob, out, overflow);
  }
  return hipGetLastError();
}
