// fg_synth_rule.h - AV1's film-grain synthesis (spec 7.18.3) for 4:2:0, all integers, for host and device (include/av1mi.h:
// av1mi_film_grain_synth): fg_synth_kernel.hip runs it, tests/host/fg_synth_rule_host.cpp compiles it for the CPU
// against the numpy restatement (tests/fgs_ref.py), which dav1d's output pins.  Normative: every step is the decoder's.
//
//   register     16 bits; a step feeds bit 0 ^ bit 1 ^ bit 3 ^ bit 12 in at the top; get_random_number(n) is one step and the top n bits
//   templates    LumaGrain 73 x 82, CbGrain and CrGrain 38 x 44, registers seeded seed, seed ^ 0xb524, seed ^ 0x49d8: every sample
//                Round2(Gaussian_Sequence[11 bits], 12 - bit_depth + grain_scale_shift) in raster order (zero for a plane without a
//                scaling function), then the autoregressive filter over rows 3 .., columns 3 .. width - 4 in raster order: the 2 L (L + 1)
//                causal neighbours at lag L, for chroma also the 2 x 2 luma mean at the co-located position, Round2 by
//                ar_coeff_shift_minus_6 + 6, clamped to GrainMin .. GrainMax
//   Round2       on signed values the arithmetic shift of x + half, as dav1d has it
//   scaling      per plane 256 entries: linear between the points (the spec's 16-bit reciprocal), flat outside them;
//                chroma_scaling_from_luma gives both chroma planes the luma function.  scale_lut interpolates it at 10 bits, not at 255
//   blocks       per stripe of 32 luma rows a register seeded seed ^ ((37 n + 178) & 255) << 8 ^ ((173 n + 105) & 255); every 32 x 32 luma
//                block one step, its top 8 bits the block's offsets: x = v >> 4, y = v & 15.  A block's noise is the 34 x 34 window of the
//                template at (9 + 2 y, 9 + 2 x), for chroma 17 x 17 at (6 + y, 6 + x): two (one) samples overlap the next block and stripe
//   overlap      a block's first two columns against the left block's last two, 27/17 and 17/27 (chroma: one column, 23/22), Round2 by 5
//                and clamped; then a stripe's first two rows against the upper stripe's last two the same way - both already blended
//                horizontally
//   blend        out = Clip3(min, max, in + Round2(scale_lut(in or merged) * noise, grain_scaling_minus_8 + 8)); chroma is indexed by
//                merged = Clip1((avg * (luma_mult - 128) + in * (mult - 128) >> 6) + (offset - 256 << bit_depth - 8)), or by avg alone with
//                chroma_scaling_from_luma; avg = Round2(Y[2y][2x] + Y[2y][min(2x + 1, w - 1)], 1) of the luma before its grain
#ifndef AV1MI_FG_SYNTH_RULE_H
#define AV1MI_FG_SYNTH_RULE_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/av1mi.h"
#include "fg_gauss_table.h"
#ifdef __HIPCC__
#define AV1MI_FGS_HD __host__ __device__
#else
#define AV1MI_FGS_HD
#endif

#define AV1MI_FGS_LUMA_W 82
#define AV1MI_FGS_LUMA_H 73
#define AV1MI_FGS_CHROMA_W 44
#define AV1MI_FGS_CHROMA_H 38
#define AV1MI_FGS_LUMA_N (AV1MI_FGS_LUMA_W * AV1MI_FGS_LUMA_H)         // 5986
#define AV1MI_FGS_CHROMA_N (AV1MI_FGS_CHROMA_W * AV1MI_FGS_CHROMA_H)   // 1672
#define AV1MI_FGS_TEMPLATE_N (AV1MI_FGS_LUMA_N + 2 * AV1MI_FGS_CHROMA_N)   // a frame's three templates, one after the other: 9330 samples

AV1MI_FGS_HD inline int av1mi_fgs_template_w(int pl) { return pl ? AV1MI_FGS_CHROMA_W : AV1MI_FGS_LUMA_W; }
AV1MI_FGS_HD inline int av1mi_fgs_template_h(int pl) { return pl ? AV1MI_FGS_CHROMA_H : AV1MI_FGS_LUMA_H; }
AV1MI_FGS_HD inline int av1mi_fgs_template_at(int pl) { return pl == 0 ? 0 : AV1MI_FGS_LUMA_N + (pl - 1) * AV1MI_FGS_CHROMA_N; }
// the stripes and the blocks of a stripe of a picture of h rows and w columns of luma
AV1MI_FGS_HD inline int av1mi_fgs_stripes(int h) { return ((h + 1) / 2 + 15) / 16; }
AV1MI_FGS_HD inline int av1mi_fgs_blocks(int w) { return ((w + 1) / 2 + 15) / 16; }

AV1MI_FGS_HD inline uint32_t av1mi_fgs_lfsr(uint32_t r) {
  const uint32_t bit = (r ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1u;
  return (r >> 1) | (bit << 15);
}
AV1MI_FGS_HD inline int av1mi_fgs_round2(int x, int n) { return (x + ((1 << n) >> 1)) >> n; }
AV1MI_FGS_HD inline int av1mi_fgs_grain_min(int bd) { return -(128 << (bd - 8)); }
AV1MI_FGS_HD inline int av1mi_fgs_grain_max(int bd) { return (256 << (bd - 8)) - 1 - (128 << (bd - 8)); }
AV1MI_FGS_HD inline int av1mi_fgs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
AV1MI_FGS_HD inline int av1mi_fgs_clamp_grain(int v, int bd) { return av1mi_fgs_clamp(v, av1mi_fgs_grain_min(bd), av1mi_fgs_grain_max(bd)); }

// whether a plane has a scaling function: its template is drawn and its samples change
AV1MI_FGS_HD inline bool av1mi_fgs_plane_on(const av1mi_grain_params &g, int pl) {
  return pl == 0 ? g.num_y_points > 0 : (g.chroma_scaling_from_luma || (pl == 1 ? g.num_cb_points : g.num_cr_points) > 0);
}
AV1MI_FGS_HD inline bool av1mi_fgs_any_plane_on(const av1mi_grain_params &g) {
  return av1mi_fgs_plane_on(g, 0) || av1mi_fgs_plane_on(g, 1) || av1mi_fgs_plane_on(g, 2);
}
// the register a plane's draws start from
AV1MI_FGS_HD inline uint32_t av1mi_fgs_plane_seed(uint32_t seed, int pl) { return seed ^ (pl == 0 ? 0u : (pl == 1 ? 0xb524u : 0x49d8u)); }
// a plane's draws: the 11-bit table indices of its n samples in raster order - the register's serial chain and nothing else
AV1MI_FGS_HD inline void av1mi_fgs_draw_indices(int pl, uint32_t seed, int16_t *t) {
  const int n = pl ? AV1MI_FGS_CHROMA_N : AV1MI_FGS_LUMA_N;
  uint32_t r = av1mi_fgs_plane_seed(seed, pl);
  for (int i = 0; i < n; i++) {
    r = av1mi_fgs_lfsr(r);
    t[i] = (int16_t)(r >> 5);
  }
}
// a template sample before the filter from its table index
AV1MI_FGS_HD inline int16_t av1mi_fgs_drawn(const av1mi_grain_params &g, int pl, int bd, int index, const int16_t *gauss) {
  return av1mi_fgs_plane_on(g, pl) ? (int16_t)av1mi_fgs_round2(gauss[index], 12 - bd + g.grain_scale_shift) : (int16_t)0;
}
// a plane's template before the filter
AV1MI_FGS_HD inline void av1mi_fgs_draw(const av1mi_grain_params &g, int pl, int bd, uint32_t seed, const int16_t *gauss, int16_t *t) {
  av1mi_fgs_draw_indices(pl, seed, t);
  for (int i = 0; i < (pl ? AV1MI_FGS_CHROMA_N : AV1MI_FGS_LUMA_N); i++) t[i] = av1mi_fgs_drawn(g, pl, bd, t[i], gauss);
}
// the filter at (y, x) of a plane's template t: every sample above and left of it within the lag filtered before; luma: the filtered luma
// template, read by the chroma planes
AV1MI_FGS_HD inline void av1mi_fgs_ar_at(const av1mi_grain_params &g, int pl, int bd, int16_t *t, const int16_t *luma, int y, int x) {
  const int lag = g.ar_coeff_lag, w = av1mi_fgs_template_w(pl);
  const int8_t *c = pl == 0 ? g.ar_coeffs_y : (pl == 1 ? g.ar_coeffs_cb : g.ar_coeffs_cr);
  int sum = 0, pos = 0;
  for (int dr = -lag; dr <= 0; dr++)
    for (int dc = -lag; dc <= lag && (dr || dc); dc++) sum += c[pos++] * t[(y + dr) * w + x + dc];
  if (pl && g.num_y_points) {
    const int16_t *l = luma + (((y - 3) << 1) + 3) * AV1MI_FGS_LUMA_W + ((x - 3) << 1) + 3;
    sum += c[pos] * av1mi_fgs_round2(l[0] + l[1] + l[AV1MI_FGS_LUMA_W] + l[AV1MI_FGS_LUMA_W + 1], 2);
  }
  t[y * w + x] = (int16_t)av1mi_fgs_clamp_grain(t[y * w + x] + av1mi_fgs_round2(sum, g.ar_coeff_shift_minus_6 + 6), bd);
}
// a frame's three templates, one after the other (av1mi_fgs_template_at), in the spec's order: what the kernel's skewed walk must equal
inline void av1mi_fgs_templates(const av1mi_grain_params &g, int bd, uint32_t seed, int16_t *t) {
  for (int pl = 0; pl < 3; pl++) {
    int16_t *p = t + av1mi_fgs_template_at(pl);
    av1mi_fgs_draw(g, pl, bd, seed, av1mi_fg_gaussian_sequence, p);
    for (int y = 3; y < av1mi_fgs_template_h(pl); y++)
      for (int x = 3; x < av1mi_fgs_template_w(pl) - 3; x++) av1mi_fgs_ar_at(g, pl, bd, p, t, y, x);
  }
}

// entry i of a plane's scaling function
AV1MI_FGS_HD inline int av1mi_fgs_scaling_entry(const av1mi_grain_params &g, int pl, int i) {
  if (pl && g.chroma_scaling_from_luma) pl = 0;
  const uint8_t (*p)[2] = pl == 0 ? g.point_y : (pl == 1 ? g.point_cb : g.point_cr);
  const int n = pl == 0 ? g.num_y_points : (pl == 1 ? g.num_cb_points : g.num_cr_points);
  if (n == 0) return 0;
  if (i < p[0][0]) return p[0][1];
  for (int k = 0; k + 1 < n; k++) {
    if (i >= p[k + 1][0]) continue;
    const int dx = p[k + 1][0] - p[k][0], dy = p[k + 1][1] - p[k][1];
    const int delta = dy * ((65536 + (dx >> 1)) / dx);
    return p[k][1] + (((i - p[k][0]) * delta + 32768) >> 16);
  }
  return p[n - 1][1];
}
// scale_lut: the function at a sample value, lut its 256 entries
template <class T>
AV1MI_FGS_HD inline int av1mi_fgs_scale_lut(const T *lut, int index, int bd) {
  const int shift = bd - 8, x = index >> shift, rem = index - (x << shift);
  if (shift == 0 || x >= 255) return lut[x > 255 ? 255 : x];   // (above 255: a sample beyond the bit depth, which no decoder hands over)
  const int start = lut[x], end = lut[x + 1];
  return start + av1mi_fgs_round2((end - start) * rem, shift);
}

// a stripe's register before its first block
AV1MI_FGS_HD inline uint32_t av1mi_fgs_stripe_seed(uint32_t seed, int n) {
  return seed ^ ((uint32_t)((n * 37 + 178) & 255) << 8) ^ (uint32_t)((n * 173 + 105) & 255);
}
// the blocks' 8-bit values of stripe n
AV1MI_FGS_HD inline void av1mi_fgs_block_offsets(uint32_t seed, int n, int blocks, uint8_t *out) {
  uint32_t r = av1mi_fgs_stripe_seed(seed, n);
  for (int b = 0; b < blocks; b++) { r = av1mi_fgs_lfsr(r); out[b] = (uint8_t)(r >> 8); }
}
// where the window of a block with value v starts in a plane's template: the sample of the block's (0, 0)
AV1MI_FGS_HD inline int av1mi_fgs_window(int v, int pl) {
  const int ox = v >> 4, oy = v & 15;
  return pl ? (6 + oy) * AV1MI_FGS_CHROMA_W + 6 + ox : (9 + 2 * oy) * AV1MI_FGS_LUMA_W + 9 + 2 * ox;
}
// one overlap sample: position k of the overlap (0, 1 luma; 0 chroma), `old` the left or upper neighbour's, g the block's own
AV1MI_FGS_HD inline int av1mi_fgs_overlap(int old, int g, int k, int chroma, int bd) {
  const int wo = chroma ? 23 : (k ? 17 : 27), wg = chroma ? 22 : (k ? 27 : 17);
  return av1mi_fgs_clamp_grain(av1mi_fgs_round2(old * wo + g * wg, 5), bd);
}
// the noise of stripe row i (0 .. 33 luma, 0 .. 16 chroma) at plane column x, blended horizontally: t the plane's template, offs the
// stripe's block values
AV1MI_FGS_HD inline int av1mi_fgs_stripe_noise(const int16_t *t, const uint8_t *offs, int pl, int i, int x, int overlap, int bd) {
  const int sh = pl ? 4 : 5, b = x >> sh, j = x - (b << sh), tw = av1mi_fgs_template_w(pl);
  int g = t[av1mi_fgs_window(offs[b], pl) + i * tw + j];
  if (overlap && b > 0 && j < (pl ? 1 : 2)) g = av1mi_fgs_overlap(t[av1mi_fgs_window(offs[b - 1], pl) + i * tw + j + (1 << sh)], g, j, pl != 0, bd);
  return g;
}
// NoiseImage[pl][y][x]: offs the frame's block values [stripe][blocks]
AV1MI_FGS_HD inline int av1mi_fgs_noise(const int16_t *t, const uint8_t *offs, int blocks, int pl, int y, int x, int overlap, int bd) {
  const int sh = pl ? 4 : 5, s = y >> sh, i = y - (s << sh);
  int g = av1mi_fgs_stripe_noise(t, offs + (size_t)s * blocks, pl, i, x, overlap, bd);
  if (overlap && s > 0 && i < (pl ? 1 : 2))
    g = av1mi_fgs_overlap(av1mi_fgs_stripe_noise(t, offs + (size_t)(s - 1) * blocks, pl, i + (1 << sh), x, overlap, bd), g, i, pl != 0, bd);
  return g;
}

// the output range: lo, and hi of a plane
AV1MI_FGS_HD inline int av1mi_fgs_out_min(const av1mi_grain_params &g, int bd) { return g.clip_to_restricted_range ? 16 << (bd - 8) : 0; }
AV1MI_FGS_HD inline int av1mi_fgs_out_max(const av1mi_grain_params &g, int pl, int bd) {
  return g.clip_to_restricted_range ? (pl == 0 || g.mc_identity ? 235 : 240) << (bd - 8) : (1 << bd) - 1;
}
// the value a chroma sample's scaling function is read at: avg the luma mean, orig the sample
AV1MI_FGS_HD inline int av1mi_fgs_merged(const av1mi_grain_params &g, int pl, int avg, int orig, int bd) {
  if (g.chroma_scaling_from_luma) return avg;
  const int lm = (pl == 1 ? g.cb_luma_mult : g.cr_luma_mult) - 128, m = (pl == 1 ? g.cb_mult : g.cr_mult) - 128;
  const int off = (pl == 1 ? g.cb_offset : g.cr_offset) - 256;
  return av1mi_fgs_clamp(((avg * lm + orig * m) >> 6) + off * (1 << (bd - 8)), 0, (1 << bd) - 1);
}
// a sample with its grain: at = the value the function is read at (the sample itself for luma), lut the plane's function
template <class T>
AV1MI_FGS_HD inline int av1mi_fgs_blend(const av1mi_grain_params &g, int pl, const T *lut, int orig, int at, int noise, int bd) {
  const int v = orig + av1mi_fgs_round2(av1mi_fgs_scale_lut(lut, at, bd) * noise, g.grain_scaling_minus_8 + 8);
  return av1mi_fgs_clamp(v, av1mi_fgs_out_min(g, bd), av1mi_fgs_out_max(g, pl, bd));
}

// what av1mi_film_grain_synth refuses: too many points, points out of order, a lag, shift or offset out of range
inline bool av1mi_fgs_params_valid(const av1mi_grain_params &g) {
  const uint8_t (*pts[3])[2] = { g.point_y, g.point_cb, g.point_cr };
  const int n[3] = { g.num_y_points, g.num_cb_points, g.num_cr_points }, most[3] = { 14, 10, 10 };
  for (int pl = 0; pl < 3; pl++) {
    if (n[pl] > most[pl]) return false;
    for (int k = 1; k < n[pl]; k++) if (pts[pl][k][0] <= pts[pl][k - 1][0]) return false;
  }
  return g.grain_scaling_minus_8 <= 3 && g.ar_coeff_lag <= 3 && g.ar_coeff_shift_minus_6 <= 3 && g.grain_scale_shift <= 3 && g.cb_offset <= 511 &&
         g.cr_offset <= 511;
}

// What the encoder's frame headers carry with film_grain = N (av1mi_syntax.cpp: make_frame_header, whose placeholders fg_table_kernel and
// fg_ar_solve_kernel overwrite): the fixed table's two points per plane, 2 N luma / N chroma - or, estimated, eight points at
// x = 16 + 32 k with table's 24 values [plane][bin] - and at a lag the fit's coefficients [plane][25] with a luma tap of 0 at shift 7;
// grain_scaling_minus_8 = 3, the chroma functions read at the luma mean (128, 192, 256), overlap on, full range
AV1MI_FGS_HD inline void av1mi_fgs_header_params(int N, int estimate, int lag, const uint8_t *table, const int8_t *coeffs, av1mi_grain_params *g) {
  uint8_t *raw = reinterpret_cast<uint8_t *>(g);
  for (size_t i = 0; i < sizeof(*g); i++) raw[i] = 0;
  uint8_t (*pts[3])[2] = { g->point_y, g->point_cb, g->point_cr };
  int8_t *co[3] = { g->ar_coeffs_y, g->ar_coeffs_cb, g->ar_coeffs_cr };
  const int n_points = estimate ? 8 : 2, n_pos = 2 * lag * (lag + 1);
  g->num_y_points = g->num_cb_points = g->num_cr_points = (uint8_t)n_points;
  for (int pl = 0; pl < 3; pl++) {
    const int fixed = pl ? N : (2 * N > 255 ? 255 : 2 * N);
    for (int k = 0; k < n_points; k++) {
      pts[pl][k][0] = (uint8_t)(estimate ? 16 + 32 * k : 255 * k);
      pts[pl][k][1] = (uint8_t)(estimate ? table[pl * 8 + k] : fixed);
    }
    for (int i = 0; i < n_pos; i++) co[pl][i] = coeffs[pl * 25 + i];
  }
  g->grain_scaling_minus_8 = 3;
  g->ar_coeff_lag = (uint8_t)lag;
  g->ar_coeff_shift_minus_6 = lag ? 1 : 0;
  g->cb_mult = g->cr_mult = 128;
  g->cb_luma_mult = g->cr_luma_mult = 192;
  g->cb_offset = g->cr_offset = 256;
  g->overlap_flag = 1;
}

// One frame on the host, plane by plane as the spec says it: in and out the tight planar frame of h x w luma (both even), t and offs
// scratch of AV1MI_FGS_TEMPLATE_N samples and stripes x blocks values.  A parameter set without a scaling function copies the frame.
template <class PIX>
inline void av1mi_fgs_frame(const av1mi_grain_params &g, int bd, uint32_t seed, const PIX *in, PIX *out, int w, int h, int16_t *t, uint8_t *offs) {
  const size_t n = (size_t)w * h * 3 / 2;
  for (size_t i = 0; i < n; i++) out[i] = in[i];
  if (!av1mi_fgs_any_plane_on(g)) return;
  av1mi_fgs_templates(g, bd, seed, t);
  const int stripes = av1mi_fgs_stripes(h), blocks = av1mi_fgs_blocks(w);
  for (int s = 0; s < stripes; s++) av1mi_fgs_block_offsets(seed, s, blocks, offs + (size_t)s * blocks);
  int lut[3][256];
  for (int pl = 0; pl < 3; pl++)
    for (int i = 0; i < 256; i++) lut[pl][i] = av1mi_fgs_scaling_entry(g, pl, i);
  for (int pl = 0; pl < 3; pl++) {
    if (!av1mi_fgs_plane_on(g, pl)) continue;
    const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h;
    const size_t at = pl == 0 ? 0 : (size_t)w * h + (pl == 2 ? (size_t)pw * ph : 0);
    for (int y = 0; y < ph; y++)
      for (int x = 0; x < pw; x++) {
        const int orig = in[at + (size_t)y * pw + x];
        int idx = orig;
        if (pl) {
          const int x1 = 2 * x + 1 < w - 1 ? 2 * x + 1 : w - 1;
          idx = av1mi_fgs_merged(g, pl, av1mi_fgs_round2(in[(size_t)2 * y * w + 2 * x] + in[(size_t)2 * y * w + x1], 1), orig, bd);
        }
        const int noise = av1mi_fgs_noise(t + av1mi_fgs_template_at(pl), offs, blocks, pl, y, x, g.overlap_flag, bd);
        out[at + (size_t)y * pw + x] = (PIX)av1mi_fgs_blend(g, pl, lut[pl], orig, idx, noise, bd);
      }
  }
}

#endif
