// fg_denoise_rule.h - the source denoised by the chunk's film-grain table before it is coded (av1mi_params.film_grain bits 8 and 10:
// AV1MI_FILM_GRAIN_DENOISE), all integers, for host and device: fg_denoise_kernel.hip runs it per sample,
// tests/host/fgd_rule_host.cpp compiles it for the CPU against the numpy restatement (tests/fgd_ref.py).  Non-normative: the decoder
// sees the table and a stream coded from the denoised frames.  One rule for the three planes.
//
//   LUT      lut_p[x], x = 0 .. 255, of plane p from its eight signalled values v_0 .. v_7 at x = 16 + 32 k (the table after the ceiling,
//            what the frame headers carry) - the decoder's scaling function: v_0 below 16, v_7 from 240 on, between them with
//            k = (x - 16) >> 5, j = (x - 16) & 31: v_k + ((j (v_{k+1} - v_k) + 16) >> 5), the shift arithmetic
//   index    always luma, of the frame as the caller gave it: Y[r][c] >> (bd - 8) for a luma sample, for a chroma sample
//            ((Y[2r][2c] + Y[2r][2c + 1] + 1) >> 1) >> (bd - 8) - with cb_mult 128, cb_luma_mult 192 and cb_offset 256 the decoder indexes
//            the chroma functions by that average (fg_rule.h)
//   reach    T = ((lut[index] << (bd - 8)) + 8) >> 4: the decoder's grain has sigma = value / 64 at 8-bit scale, T is 4 sigma at the stream's
//            bit depth, at most 16 (8 bits) / 64 (10 bits).  T = 0: the sample is copied
//   filter   over the 5x5 window around the sample, coordinates clamped to the plane's signalled picture: w_i = max(0, T - |x_i - x_c|) (the
//            centre weighs T), out = (sum w_i x_i + den / 2) / den, den = sum w_i <= 25 * 64; the numerator stays below 2^21
//   so       a zero table is the identity; |out - x_c| <= max(0, T - 1); a constant plane and a sample whose neighbours all differ from it
//            by at least T are unchanged
//   padding  samples of the coded size outside the signalled picture replicate the DENOISED edge
#ifndef AV1MI_FG_DENOISE_RULE_H
#define AV1MI_FG_DENOISE_RULE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_FGD_HD __host__ __device__
#else
#define AV1MI_FGD_HD
#endif

#define AV1MI_FGD_RADIUS 2
#define AV1MI_FGD_MAX_REACH 64

// lut_p[x] from the plane's eight values
AV1MI_FGD_HD inline int av1mi_fgd_lut(const uint8_t *v, int x) {
  if (x < 16) return v[0];
  if (x >= 240) return v[7];
  const int k = (x - 16) >> 5, j = (x - 16) & 31;
  return (int)v[k] + ((j * ((int)v[k + 1] - (int)v[k]) + 16) >> 5);
}
// the index of a luma sample, and of a chroma sample from the two luma samples of its row pair's upper row
AV1MI_FGD_HD inline int av1mi_fgd_index_luma(int y, int bit_depth) { return y >> (bit_depth - 8); }
AV1MI_FGD_HD inline int av1mi_fgd_index_chroma(int y0, int y1, int bit_depth) { return ((y0 + y1 + 1) >> 1) >> (bit_depth - 8); }
// T from the LUT's value
AV1MI_FGD_HD inline int av1mi_fgd_reach(int lut, int bit_depth) { return ((lut << (bit_depth - 8)) + 8) >> 4; }
// one sample of the window into the sums
AV1MI_FGD_HD inline void av1mi_fgd_tap(int T, int xc, int xi, uint32_t &num, uint32_t &den) {
  const int d = xi < xc ? xc - xi : xi - xc;
  const uint32_t w = d < T ? (uint32_t)(T - d) : 0u;
  den += w;
  num += w * (uint32_t)xi;
}
// the sample from the sums (den = 0: T = 0, the copy)
AV1MI_FGD_HD inline int av1mi_fgd_out(int xc, uint32_t num, uint32_t den) { return den ? (int)((num + den / 2) / den) : xc; }
// the filter at (r, c) of a w x h plane at x[row * stride + column] with reach T
template <class PIX>
AV1MI_FGD_HD inline int av1mi_fgd_sample(const PIX *x, size_t stride, int w, int h, int r, int c, int T) {
  const int xc = x[(size_t)r * stride + c];
  uint32_t num = 0, den = 0;
  for (int dy = -AV1MI_FGD_RADIUS; dy <= AV1MI_FGD_RADIUS; dy++)
    for (int dx = -AV1MI_FGD_RADIUS; dx <= AV1MI_FGD_RADIUS; dx++) {
      const int rr = r + dy < 0 ? 0 : (r + dy >= h ? h - 1 : r + dy), cc = c + dx < 0 ? 0 : (c + dx >= w ? w - 1 : c + dx);
      av1mi_fgd_tap(T, xc, x[(size_t)rr * stride + cc], num, den);
    }
  return av1mi_fgd_out(xc, num, den);
}

#endif
