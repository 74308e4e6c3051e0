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
//
// The temporal term (bits 14 and 15 with bits 8 and 10: AV1MI_FILM_GRAIN_DENOISE_TEMPORAL).  Grain is independent from
// frame to frame, picture content is not: frame f's filter also takes the same sample of its neighbours g = f - S .. f + S (S = 1, with bit 9
// S = 2; g != f, 0 <= g < n_frames, across key frames), along the motion.  The spatial taps are untouched.
//   search   per 16x16 luma block of the coded grid the whole-sample full search of +-R of frame f in frame g (tf_search.h, me_rule.h's reach,
//            cost, index and node key), on the undenoised frames at the coded size; key (cost << 11) | index, all-ones for a neighbour that
//            does not exist, at mv[(f * 4 + slot) * nb + b], slots 0 .. 3 = g - f = -2, -1, +1, +2
//   block    of a sample (r, c): (r >> 4, c >> 4) for luma, (r >> 3, c >> 3) for chroma; (dx, dy) from that block's index for g
//   window   3x3 around (r + dy, c + dx) of the caller's UNDENOISED frame g - chroma: around (r + (dy >> 1), c + (dx >> 1)), the shifts
//            arithmetic, whole samples - the nine coordinates clamped one by one to the plane's signalled picture; every tap with the
//            frame-f sample's T and x_c, the centre weighing 4 w, the eight around it w: a wrong match weighs nothing
//   so       den <= 1600 + 2 S * 12 * 64 (4672 at S = 2), num <= 4672 * 1023 < 2^23; a zero table is still the identity and
//            |out - x_c| <= max(0, T - 1) still holds; a one-frame chunk is the spatial filter; a sample past the signalled picture is the
//            one at the clamped position, with the block of the clamped position
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
#define AV1MI_FGD_SLOTS 4            // the neighbours' slots of a frame: g - f = -2, -1, +1, +2
#define AV1MI_FGD_CENTRE_WEIGHT 4    // the temporal window's centre tap weighs so many times its neighbours
#define AV1MI_FGD_NONE 0xFFFFFFFFu   // the key of a neighbour that does not exist (me_rule.h: AV1MI_ME_NODE_NONE)

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
// ... k times: the temporal window's centre
AV1MI_FGD_HD inline void av1mi_fgd_tap_times(int k, int T, int xc, int xi, uint32_t &num, uint32_t &den) {
  const int d = xi < xc ? xc - xi : xi - xc;
  const uint32_t w = d < T ? (uint32_t)(k * (T - d)) : 0u;
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

// ---- the temporal term
// the field's span: 0 without bits 14 and 15, else 1, with bit 9 2 (include/av1mi.h: AV1MI_FILM_GRAIN_DENOISE_SPAN)
AV1MI_FGD_HD inline int av1mi_fgd_field_span(uint32_t v) { return (v & 0xC000u) == 0xC000u ? ((v & 0x200u) ? 2 : 1) : 0; }
// frame g - f of a slot, and whether frame f of n_frames has that neighbour at span S
AV1MI_FGD_HD inline int av1mi_fgd_slot_offset(int slot) { return slot < 2 ? slot - 2 : slot - 1; }
AV1MI_FGD_HD inline bool av1mi_fgd_slot_exists(int f, int slot, int span, int n_frames) {
  const int o = av1mi_fgd_slot_offset(slot), g = f + o;
  return (o < 0 ? -o : o) <= span && g >= 0 && g < n_frames;
}
// the vector of a key's index at range R, and the component a chroma window moves by (av1mi_tf_chroma_base: d >> 1, arithmetic)
AV1MI_FGD_HD inline void av1mi_fgd_vector(uint32_t key, int R, int *dy, int *dx) {
  const int nc = 2 * R + 1, i = (int)(key & 0x7FFu);
  *dy = i / nc - R; *dx = i % nc - R;
}
AV1MI_FGD_HD inline int av1mi_fgd_chroma_shift(int d) { return d >> 1; }
// the 3x3 window of neighbour frame's plane y (w x h, rows `stride` apart) around (r, c) into the sums of a sample with reach T and centre xc
template <class PIX>
AV1MI_FGD_HD inline void av1mi_fgd_window(const PIX *y, size_t stride, int w, int h, int r, int c, int T, int xc, uint32_t &num, uint32_t &den) {
  for (int v = -1; v <= 1; v++)
    for (int u = -1; u <= 1; u++) {
      const int rr = r + v < 0 ? 0 : (r + v >= h ? h - 1 : r + v), cc = c + u < 0 ? 0 : (c + u >= w ? w - 1 : c + u);
      av1mi_fgd_tap_times(v == 0 && u == 0 ? AV1MI_FGD_CENTRE_WEIGHT : 1, T, xc, y[(size_t)rr * stride + cc], num, den);
    }
}
// the filter at (r, c) of plane x of frame f with reach T and its neighbours: nbr[slot] the same plane of the slot's frame or null,
// key[slot] that frame's key of the sample's block; chroma: the plane is a chroma plane
template <class PIX>
AV1MI_FGD_HD inline int av1mi_fgd_sample_temporal(const PIX *x, const PIX *const *nbr, const uint32_t *key, int R, int chroma, size_t stride, int w, int h,
                                                  int r, int c, int T, uint32_t *num_out = nullptr, uint32_t *den_out = nullptr) {
  const int xc = x[(size_t)r * stride + c];
  uint32_t num = 0, den = 0;
  for (int dy = -AV1MI_FGD_RADIUS; dy <= AV1MI_FGD_RADIUS; dy++)
    for (int dx = -AV1MI_FGD_RADIUS; dx <= AV1MI_FGD_RADIUS; dx++) {
      const int rr = r + dy < 0 ? 0 : (r + dy >= h ? h - 1 : r + dy), cc = c + dx < 0 ? 0 : (c + dx >= w ? w - 1 : c + dx);
      av1mi_fgd_tap(T, xc, x[(size_t)rr * stride + cc], num, den);
    }
  for (int s = 0; s < AV1MI_FGD_SLOTS; s++) {
    if (!nbr[s] || key[s] == AV1MI_FGD_NONE) continue;
    int dy, dx;
    av1mi_fgd_vector(key[s], R, &dy, &dx);
    if (chroma) { dy = av1mi_fgd_chroma_shift(dy); dx = av1mi_fgd_chroma_shift(dx); }
    av1mi_fgd_window(nbr[s], stride, w, h, r + dy, c + dx, T, xc, num, den);
  }
  if (num_out) *num_out = num;
  if (den_out) *den_out = den;
  return av1mi_fgd_out(xc, num, den);
}

#endif
