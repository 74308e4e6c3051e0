// fg_synth_kernel.hip - the film-grain synthesis pass: what a decoder adds to a chunk's frames (include/av1mi.h:
// av1mi_film_grain_synth, av1mi_ctx_set_displayed_quality; fg_synth_rule.h is the rule).
//
// fgs_template_kernel, a workgroup per frame: the three templates in LDS.  One lane per plane steps the plane's register - a serial
// chain, nothing else on it - and leaves the table indices, which all lanes then look up.  The filter runs rows on lanes: row r works on
// column x at step x + r (lag + 1), so that every sample above and left of it within the lag is done, 76 + 69 (lag + 1) steps for luma's
// 70 rows instead of 5 320; the chroma planes follow, they read the filtered luma.  The same workgroup fills the frame's block values,
// the first also the three scaling functions.  Both kernels read the parameter set from device memory: inside the encoder
// fgs_params_kernel forms it from the estimate's and the fit's results where they stand.
// fgs_apply_kernel, a workgroup per run of eight 32x32 blocks of a stripe: a lane takes 8 luma samples of two rows and the 4 U and 4 V
// samples under them, twice - rows of 256 samples a wave, every sample read once and written once (the chroma planes index their function
// by the luma the lane holds).  The noise comes straight from the templates, 19 KB a frame which the caches hold; the functions are in LDS.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "fg_synth_rule.h"

namespace {

__device__ __forceinline__ uint32_t frame_seed(const uint16_t *seeds, uint32_t first_frame, int f) {
  return seeds ? seeds[f] : (7391u + 173u * (first_frame + (uint32_t)f)) & 0xFFFFu;
}

// the filter of planes pl0 .. pl0 + planes - 1, each plane's rows on lanes of their own
__device__ __forceinline__ void ar_walk(const av1mi_grain_params &g, int bd, int16_t *t, int pl0, int planes, int tid) {
  const int rows = av1mi_fgs_template_h(pl0) - 3, cols = av1mi_fgs_template_w(pl0) - 6, skew = g.ar_coeff_lag + 1;
  const int pl = pl0 + tid / rows, r = tid % rows;
  const bool lane = tid < rows * planes;
  for (int step = 0; step < cols + (rows - 1) * skew; step++) {
    const int x = step - r * skew;
    if (lane && x >= 0 && x < cols) av1mi_fgs_ar_at(g, pl, bd, t + av1mi_fgs_template_at(pl), t, 3 + r, 3 + x);
    __syncthreads();
  }
}

__global__ void fgs_params_kernel(int N, int estimate, int lag, const uint8_t *__restrict__ table, const int8_t *__restrict__ coeffs, Av1miFgsBlock B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) av1mi_fgs_header_params(N, estimate, lag, table, coeffs, B.g);
}

// grid (x = frame)
__global__ void __launch_bounds__(256) fgs_template_kernel(int bd, int w, int h, const uint16_t *__restrict__ seeds, uint32_t first_frame, Av1miFgsBlock B) {
  __shared__ int16_t t[AV1MI_FGS_TEMPLATE_N];
  __shared__ av1mi_grain_params g;   // (the filter indexes the coefficients)
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < (int)sizeof(g)) reinterpret_cast<uint8_t *>(&g)[tid] = reinterpret_cast<const uint8_t *>(B.g)[tid];
  __syncthreads();
  const uint32_t seed = frame_seed(seeds, first_frame, f);
  // the draws: one lane per plane steps the register and leaves the table indices - nothing but the chain - then every lane looks its samples up
  if ((tid & 63) == 0 && tid < 192) av1mi_fgs_draw_indices(tid >> 6, seed, t + av1mi_fgs_template_at(tid >> 6));
  __syncthreads();
  for (int i = tid; i < AV1MI_FGS_TEMPLATE_N; i += 256)
    t[i] = av1mi_fgs_drawn(g, i < AV1MI_FGS_LUMA_N ? 0 : (i < AV1MI_FGS_LUMA_N + AV1MI_FGS_CHROMA_N ? 1 : 2), bd, t[i], av1mi_fg_gaussian_sequence);
  __syncthreads();
  ar_walk(g, bd, t, 0, 1, tid);
  ar_walk(g, bd, t, 1, 2, tid);
  int16_t *out = B.templates + (size_t)f * AV1MI_FGS_TEMPLATE_N;
  for (int i = tid; i < AV1MI_FGS_TEMPLATE_N; i += 256) out[i] = t[i];
  const int stripes = av1mi_fgs_stripes(h), blocks = av1mi_fgs_blocks(w);
  for (int s = tid; s < stripes; s += 256) av1mi_fgs_block_offsets(seed, s, blocks, B.offs + ((size_t)f * stripes + s) * blocks);
  if (f == 0)
    for (int pl = 0; pl < 3; pl++) B.lut[pl * 256 + tid] = (uint8_t)av1mi_fgs_scaling_entry(g, pl, tid);
}

// N samples of a row at p, of which the first n lie inside the plane: one load where all do and the address allows it
template <typename PIX, int N>
__device__ __forceinline__ void load_row(const PIX *__restrict__ p, int n, int v[N]) {
  typedef PIX Vec __attribute__((ext_vector_type(N)));
  if (n == N && (reinterpret_cast<uintptr_t>(p) & (N * sizeof(PIX) - 1)) == 0) {
    const Vec x = *reinterpret_cast<const Vec *>(p);
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = x[k];
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = k < n ? (int)p[k] : 0;
  }
}
template <typename PIX, int N>
__device__ __forceinline__ void store_row(PIX *__restrict__ p, int n, const int v[N]) {
  typedef PIX Vec __attribute__((ext_vector_type(N)));
  if (n == N && (reinterpret_cast<uintptr_t>(p) & (N * sizeof(PIX) - 1)) == 0) {
    Vec x;
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = (PIX)v[k];
    *reinterpret_cast<Vec *>(p) = x;
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) if (k < n) p[k] = (PIX)v[k];
  }
}

// N samples of NoiseImage row y of plane pl from column x0, a multiple of N inside one block: the rule's av1mi_fgs_noise, the block's
// values and windows looked up once
template <int N>
__device__ __forceinline__ void stripe_row(const int16_t *__restrict__ t, const uint8_t *__restrict__ offs, int pl, int i, int x0, int overlap, int bd, int v[N]) {
  const int sh = pl ? 4 : 5, b = x0 >> sh, j0 = x0 - (b << sh), tw = av1mi_fgs_template_w(pl);
  const int16_t *p = t + av1mi_fgs_window(offs[b], pl) + i * tw + j0;
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = p[k];
  if (overlap && b > 0 && j0 == 0) {
    const int16_t *q = t + av1mi_fgs_window(offs[b - 1], pl) + i * tw + (1 << sh);
    for (int k = 0; k < (pl ? 1 : 2); k++) v[k] = av1mi_fgs_overlap(q[k], v[k], k, pl != 0, bd);
  }
}
template <int N>
__device__ __forceinline__ void noise_row(const int16_t *__restrict__ t, const uint8_t *__restrict__ offs, int blocks, int pl, int y, int x0, int overlap, int bd, int v[N]) {
  const int sh = pl ? 4 : 5, s = y >> sh, i = y - (s << sh);
  stripe_row<N>(t, offs + (size_t)s * blocks, pl, i, x0, overlap, bd, v);
  if (overlap && s > 0 && i < (pl ? 1 : 2)) {
    int old[N];
    stripe_row<N>(t, offs + (size_t)(s - 1) * blocks, pl, i + (1 << sh), x0, overlap, bd, old);
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = av1mi_fgs_overlap(old[k], v[k], i, pl != 0, bd);
  }
}

constexpr int RUN_ITEMS = 32;   // a workgroup's items along a row: 8 luma samples each, eight blocks

// grid (x = the runs of a stripe, y = stripe, z = frame)
template <typename PIX>
__global__ void __launch_bounds__(256) fgs_apply_kernel(Av1miQualityGeom G, Av1miQualityGeom Gout, const PIX *__restrict__ in, PIX *__restrict__ out,
                                                        Av1miFgsBlock B) {
  __shared__ uint8_t lut[3 * 256];
  const av1mi_grain_params g = *B.g;   // (uniform reads; the fields the blend uses stay in registers)
  const int tid = threadIdx.x, f = blockIdx.z, bd = G.bit_depth;
  for (int i = tid; i < 3 * 256; i += 256) lut[i] = B.lut[i];
  __syncthreads();
  const int w = G.w[0], h = G.h[0], blocks = av1mi_fgs_blocks(w), stripes = av1mi_fgs_stripes(h);
  const int16_t *t = B.templates + (size_t)f * AV1MI_FGS_TEMPLATE_N;
  const uint8_t *offs = B.offs + (size_t)f * stripes * blocks;
  const PIX *src = in + (size_t)f * G.frame_samples;
  PIX *dst = out + (size_t)f * Gout.frame_samples;
  const bool on[3] = { av1mi_fgs_plane_on(g, 0), av1mi_fgs_plane_on(g, 1), av1mi_fgs_plane_on(g, 2) };
  for (int item = tid; item < RUN_ITEMS * 16; item += 256) {
    const int cy = blockIdx.y * 16 + item / RUN_ITEMS, cx0 = (blockIdx.x * RUN_ITEMS + item % RUN_ITEMS) * 4;
    const int y0 = 2 * cy, x0 = 2 * cx0;
    if (y0 >= h || x0 >= w) continue;
    const int n = w - x0 < 8 ? w - x0 : 8;   // (even: the width is)
    int top[8];
#pragma unroll
    for (int r = 0; r < 2; r++) {   // (the height is even: both rows exist)
      const size_t at = G.off[0] + (size_t)(y0 + r) * G.stride[0] + x0;
      int v[8], nz[8];
      load_row<PIX, 8>(src + at, n, v);
      if (r == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) top[k] = v[k];
      }
      if (on[0]) {
        noise_row<8>(t, offs, blocks, 0, y0 + r, x0, g.overlap_flag, bd, nz);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = av1mi_fgs_blend(g, 0, lut, v[k], v[k], nz[k], bd);
      }
      store_row<PIX, 8>(dst + Gout.off[0] + (size_t)(y0 + r) * Gout.stride[0] + x0, n, v);
    }
#pragma unroll
    for (int pl = 1; pl < 3; pl++) {
      const size_t at = G.off[pl] + (size_t)cy * G.stride[pl] + cx0;
      int v[4], nz[4];
      load_row<PIX, 4>(src + at, n / 2, v);
      if (on[pl]) {
        noise_row<4>(t + av1mi_fgs_template_at(pl), offs, blocks, pl, cy, cx0, g.overlap_flag, bd, nz);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int avg = av1mi_fgs_round2(top[2 * k] + top[2 * k + 1], 1);   // (2x + 1 <= w - 1 at an even width)
          v[k] = av1mi_fgs_blend(g, pl, lut + pl * 256, v[k], av1mi_fgs_merged(g, pl, avg, v[k], bd), nz[k], bd);
        }
      }
      store_row<PIX, 4>(dst + Gout.off[pl] + (size_t)cy * Gout.stride[pl] + cx0, n / 2, v);
    }
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_fg_synth_params(int N, int estimate, int lag, const uint8_t *table, const int8_t *coeffs, Av1miFgsBlock B, hipStream_t stream) {
  if (N < 1 || N > 255 || lag < 0 || lag > 3 || (estimate && !table) || (lag && !coeffs)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fgs_params_kernel, dim3(1), dim3(64), 0, stream, N, estimate, lag, table, coeffs, B);
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_fg_synth_templates(int bit_depth, int w, int h, int n_frames, const uint16_t *seeds, uint32_t first_frame, Av1miFgsBlock B,
                                                      hipStream_t stream) {
  if (w <= 0 || h <= 0 || ((w | h) & 1) || n_frames <= 0 || n_frames > 65535 || (bit_depth != 8 && bit_depth != 10)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fgs_template_kernel, dim3((unsigned)n_frames), dim3(256), 0, stream, bit_depth, w, h, seeds, first_frame, B);
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_fg_synth_apply(const Av1miQualityGeom *Gin, const Av1miQualityGeom *Gout, const void *in, void *out, int n_frames,
                                                  Av1miFgsBlock B, hipStream_t stream) {
  const int w = Gin->w[0], h = Gin->h[0];
  if (w <= 0 || h <= 0 || ((w | h) & 1) || n_frames <= 0 || n_frames > 65535 || in == out || Gin->bit_depth != Gout->bit_depth) return hipErrorInvalidValue;
  for (const Av1miQualityGeom *G : { Gin, Gout })
    for (int pl = 0; pl < 3; pl++)
      if (G->stride[pl] < G->w[pl] || G->w[pl] != (pl ? w / 2 : w) || G->h[pl] != (pl ? h / 2 : h)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((w + RUN_ITEMS * 8 - 1) / (RUN_ITEMS * 8)), (unsigned)av1mi_fgs_stripes(h), (unsigned)n_frames);
  if (grid.y > 65535) return hipErrorInvalidValue;
  if (Gin->bit_depth == 8) hipLaunchKernelGGL(fgs_apply_kernel<uint8_t>, grid, dim3(256), 0, stream, *Gin, *Gout, (const uint8_t *)in, (uint8_t *)out, B);
  else hipLaunchKernelGGL(fgs_apply_kernel<uint16_t>, grid, dim3(256), 0, stream, *Gin, *Gout, (const uint16_t *)in, (uint16_t *)out, B);
  return hipGetLastError();
}
