// quality_kernel.hip - the quality pass: SSIM and exact squared error of one chunk against another, per frame and plane
// (include/av1mi.h: av1mi_quality, av1mi_ctx_set_quality; ssim_rule.h is the rule).
//
// One launch covers a chunk.  A workgroup takes a (frame, plane, 64x64 tile): every 4x4 cell's sums (s1, s2, ss, s12) are formed once
// into LDS - the tile's 16 x 16 cells and one halo column and row, since a window is 2 x 2 cells and a window whose origin lies in the
// tile reaches one cell beyond it - then one lane per window adds four cells and applies the rule.  The tile's own cells also give its
// share of the squared error, ss - 2 s12.  The sums are integers added with 64-bit atomics, one per wave and quantity: any order gives
// the same result.  HBM-bound: both chunks are read once (the halo cells again, 13 % more, from the caches); algorithmic bytes 2 S b per
// frame pair (S samples of three planes, b bytes each).
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "ssim_rule.h"

namespace {

constexpr int QT_CELLS = 16, QT_LD = QT_CELLS + 1;   // a tile's cells each way, and with the halo

// four samples as one load holds them: a 32-bit word of 8-bit samples, two of 16-bit samples
__device__ __forceinline__ void unpack4(uint32_t x, uint32_t v[4]) { v[0] = x & 0xFF; v[1] = (x >> 8) & 0xFF; v[2] = (x >> 16) & 0xFF; v[3] = x >> 24; }
__device__ __forceinline__ void unpack4(uint2 x, uint32_t v[4]) { v[0] = x.x & 0xFFFF; v[1] = x.x >> 16; v[2] = x.y & 0xFFFF; v[3] = x.y >> 16; }
template <typename PIX> struct Row4;
template <> struct Row4<uint8_t> { typedef uint32_t type; };
template <> struct Row4<uint16_t> { typedef uint2 type; };
template <typename PIX>
__device__ __forceinline__ bool row4_aligned(const PIX *p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(PIX) - 1)) == 0; }

// four samples of a row at p, of which the first n (1 .. 4) lie inside the plane: one load where all four do and the address allows
// it - rows of a tight chroma plane at an odd width are not 4-byte aligned - else sample by sample; the rest count as 0
template <typename PIX>
__device__ __forceinline__ void load_row4(const PIX *__restrict__ p, int n, uint32_t v[4]) {
  if (n >= 4 && row4_aligned(p)) {
    unpack4(*reinterpret_cast<const typename Row4<PIX>::type *>(p), v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = k < n ? (uint32_t)p[k] : 0u;
  }
}

template <typename PIX>
__device__ __forceinline__ void add_row4(const uint32_t va[4], const uint32_t vb[4], uint32_t &s1, uint32_t &s2, uint32_t &ss, uint32_t &s12) {
#pragma unroll
  for (int k = 0; k < 4; k++) { s1 += va[k]; s2 += vb[k]; ss += va[k] * va[k] + vb[k] * vb[k]; s12 += va[k] * vb[k]; }
}

// the sums of the 4x4 cell at (x0, y0) of planes a and b, h x w samples with rows `stride` apart: samples outside the plane count nothing
template <typename PIX>
__device__ __forceinline__ void cell_sums(const PIX *__restrict__ pa, const PIX *__restrict__ pb, int stride, int w, int h, int x0, int y0,
                                          uint32_t &s1, uint32_t &s2, uint32_t &ss, uint32_t &s12) {
  s1 = s2 = ss = s12 = 0;
  if (x0 >= w || y0 >= h) return;
  const size_t at0 = (size_t)y0 * stride + x0;
  // the common case - the cell inside the plane, every row's address as aligned as the first's: eight loads issued together, then the sums
  if (x0 + 4 <= w && y0 + 4 <= h && (stride & 3) == 0 && row4_aligned(pa + at0) && row4_aligned(pb + at0)) {
    typedef typename Row4<PIX>::type V;
    V xa[4], xb[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      xa[r] = *reinterpret_cast<const V *>(pa + at0 + (size_t)r * stride);
      xb[r] = *reinterpret_cast<const V *>(pb + at0 + (size_t)r * stride);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      uint32_t va[4], vb[4];
      unpack4(xa[r], va);
      unpack4(xb[r], vb);
      add_row4<PIX>(va, vb, s1, s2, ss, s12);
    }
    return;
  }
  const int n = w - x0 < 4 ? w - x0 : 4;
  for (int r = 0; r < 4 && y0 + r < h; r++) {
    const size_t at = at0 + (size_t)r * stride;
    uint32_t va[4], vb[4];
    load_row4(pa + at, n, va);
    load_row4(pb + at, n, vb);
    add_row4<PIX>(va, vb, s1, s2, ss, s12);
  }
}

__device__ __forceinline__ int plane_tiles(const Av1miQualityGeom &G, int pl) { return ((G.w[pl] + 63) >> 6) * ((G.h[pl] + 63) >> 6); }

// grid (x = the tiles of the three planes one after the other, y = frame)
template <typename PIX>
__global__ void __launch_bounds__(256) quality_kernel(Av1miQualityGeom G, const PIX *__restrict__ a, const PIX *__restrict__ b,
                                                     unsigned long long *__restrict__ sums, int32_t *__restrict__ map) {
  __shared__ uint32_t cs[4][QT_LD * QT_LD];
  int t = blockIdx.x, pl = 0;
  for (; pl < 2; pl++) {
    const int n = plane_tiles(G, pl);
    if (t < n) break;
    t -= n;
  }
  const int f = blockIdx.y, tid = threadIdx.x;
  const int w = G.w[pl], h = G.h[pl], stride = G.stride[pl];
  const int tcols = (w + 63) >> 6, tx = t % tcols, ty = t / tcols;
  const size_t base = (size_t)f * G.frame_samples + G.off[pl];
  const PIX *pa = a + base, *pb = b + base;
  // the cells: every thread its own of the tile, the first 33 threads a halo cell as well - row 16, then column 16
  unsigned long long sse = 0;
  for (int k = tid; k < QT_LD * QT_LD; k += 256) {
    const int j = k - 256;
    const int r = k < 256 ? k >> 4 : (j < QT_LD ? QT_CELLS : j - QT_LD), c = k < 256 ? k & 15 : (j < QT_LD ? j : QT_CELLS);
    uint32_t s1, s2, ss, s12;
    cell_sums(pa, pb, stride, w, h, (tx * QT_CELLS + c) * 4, (ty * QT_CELLS + r) * 4, s1, s2, ss, s12);
    const int at = r * QT_LD + c;
    cs[0][at] = s1; cs[1][at] = s2; cs[2][at] = ss; cs[3][at] = s12;
    if (k < 256) sse += ss - 2 * s12;   // sum (a - b)^2 of the cell
  }
  __syncthreads();
  // the windows: one lane each
  const int ny = av1mi_ssim_windows(h), nx = av1mi_ssim_windows(w);
  const int r = tid >> 4, c = tid & 15, wy = ty * QT_CELLS + r, wx = tx * QT_CELLS + c;
  long long ssim = 0;
  if (wy < ny && wx < nx) {
    uint32_t s[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t *p = &cs[q][r * QT_LD + c];
      s[q] = p[0] + p[1] + p[QT_LD] + p[QT_LD + 1];
    }
    const int32_t v = av1mi_ssim_window(s[0], s[1], s[2], s[3], G.bit_depth);
    ssim = v;
    if (map) map[(size_t)f * G.map_frame + G.map_at[pl] + (size_t)wy * nx + wx] = v;
  }
  unsigned long long q = (unsigned long long)ssim;   // two's complement: the atomic's wrap-around is the signed sum
  for (int o = 32; o > 0; o >>= 1) { sse += __shfl_xor(sse, o, 64); q += __shfl_xor(q, o, 64); }
  if ((tid & 63) == 0) {
    unsigned long long *out = sums + ((size_t)f * 3 + pl) * 2;
    if (sse) atomicAdd(out, sse);
    if (q) atomicAdd(out + 1, q);
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_quality(const Av1miQualityGeom *G, const void *a, const void *b, int n_frames, unsigned long long *sums,
                                           int32_t *map, hipStream_t stream) {
  long tiles = 0;
  for (int pl = 0; pl < 3; pl++) {
    if (G->w[pl] <= 0 || G->h[pl] <= 0 || G->stride[pl] < G->w[pl]) return hipErrorInvalidValue;
    tiles += (long)((G->w[pl] + 63) >> 6) * ((G->h[pl] + 63) >> 6);
  }
  if (n_frames <= 0 || n_frames > 65535 || tiles > 0x7FFFFFFFl) return hipErrorInvalidValue;
  dim3 grid((unsigned)tiles, (unsigned)n_frames);
  if (G->bit_depth == 8) hipLaunchKernelGGL(quality_kernel<uint8_t>, grid, dim3(256), 0, stream, *G, (const uint8_t *)a, (const uint8_t *)b, sums, map);
  else hipLaunchKernelGGL(quality_kernel<uint16_t>, grid, dim3(256), 0, stream, *G, (const uint16_t *)a, (const uint16_t *)b, sums, map);
  return hipGetLastError();
}
