// fg_rule.h - the film-grain estimate (av1mi_params.film_grain bit 8: AV1MI_FILM_GRAIN_ESTIMATE), all integers, for
// host and device: fg_kernel.hip runs it per block and per chunk, tests/host/fg_rule_host.cpp compiles it for the CPU against the numpy
// restatement (tests/fg_ref.py).  Non-normative: the decoder only sees the table of the frame headers.
//
//   block        16x16 luma samples with their co-located 8x8 U and V samples; only blocks wholly inside the signalled picture count,
//                floor(width / 16) x floor(height / 16) per frame (padding replicates samples and would read as noiseless), of every
//                frame of the chunk, as the caller gave them (before the key frames' temporal filter)
//   bin          S = the sum of the block's 256 luma samples, m = (S + 128) >> 8, bin = (m >> (bit_depth - 8)) >> 5: 0 .. 7.  Chroma blocks
//                take their luma block's bin: with cb_mult 128, cb_luma_mult 192 and cb_offset 256 the decoder indexes the chroma
//                function by luma (spec 7.18.3.5: merged = averageLuma)
//   block value  Nsum = sum |M * x| over the interior positions (14x14 luma, 6x6 chroma), M = [1 -2 1; -2 4 -2; 1 -2 1] - Immerkaer's
//                operator, blind to planes and ramps; v = min(255, (Nsum K) >> (8 + bit_depth)), K = 4470 luma / 24336 chroma, the
//                product in 64 bits (a 10-bit checkerboard reaches 196 * 8 * 1023 * 4470).  K: sigma ~ sqrt(pi / 2) / 6 * Nsum / positions, and
//                with grain_scaling_minus_8 = 3 and AR lag 0 the decoder's grain has sigma = value / 64 at 8-bit scale, so
//                value = 64 sqrt(pi / 2) / 6 / positions * Nsum at 8-bit scale = K / 65536 * Nsum: 4470 / 65536 = 13.369 / 196,
//                24336 / 65536 = 13.369 / 36
//   table        per plane and bin the blocks' values: a bin with at least 16 blocks is populated, its value the lower quartile - the
//                smallest v whose cumulative count reaches (n + 3) / 4 (texture only inflates v: the low quantile tracks the flattest
//                blocks); an unpopulated bin takes the nearest populated bin's value, the lower index on a tie; no bin populated: all 0;
//                then the clamp to the ceiling, 2 N luma / N chroma - the fixed table's values
//   points       x = 16 + 32 k, k = 0 .. 7, eight per plane whatever the content: the header's length does not depend on it
#ifndef AV1MI_FG_RULE_H
#define AV1MI_FG_RULE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_FG_HD __host__ __device__
#else
#define AV1MI_FG_HD
#endif

#define AV1MI_FG_BLOCK 16
#define AV1MI_FG_BINS 8
#define AV1MI_FG_MIN_BLOCKS 16
#define AV1MI_FG_K_LUMA 4470u
#define AV1MI_FG_K_CHROMA 24336u
#define AV1MI_FG_MAX_N 50
#define AV1MI_FG_TABLE (3 * AV1MI_FG_BINS)   /* entries of a table and of its counts: [plane][bin] */
// film_grain_params with the estimate: eight points per plane, and how far the first cb / cr point lies behind the first luma point -
// 8 luma points of 16 bits, chroma_scaling_from_luma, num_cb_points; 8 cb points, num_cr_points
#define AV1MI_FG_CB_BIT (8 * 16 + 1 + 4)
#define AV1MI_FG_CR_BIT (AV1MI_FG_CB_BIT + 8 * 16 + 4)

// the whole blocks of an axis of `size` signalled samples
AV1MI_FG_HD inline int av1mi_fg_blocks(int size) { return size / AV1MI_FG_BLOCK; }
// x of point k
AV1MI_FG_HD inline int av1mi_fg_point_x(int k) { return 16 + 32 * k; }
// the ceiling of a plane's values with film_grain = N: what the fixed table holds
AV1MI_FG_HD inline int av1mi_fg_ceiling(int N, int plane) { return plane ? N : (2 * N > 255 ? 255 : 2 * N); }

// bin of a block from its luma sum
AV1MI_FG_HD inline int av1mi_fg_bin(uint32_t S, int bit_depth) { return (int)((((S + 128u) >> 8) >> (bit_depth - 8)) >> 5); }
// v of a block from its Nsum
AV1MI_FG_HD inline int av1mi_fg_value(uint32_t nsum, int chroma, int bit_depth) {
  const uint64_t v = ((uint64_t)nsum * (chroma ? AV1MI_FG_K_CHROMA : AV1MI_FG_K_LUMA)) >> (8 + bit_depth);
  return v > 255 ? 255 : (int)v;
}
// |M * x| at one position from its 3x3 neighbourhood: rows a (above), b, c (below), each three samples from the left
AV1MI_FG_HD inline uint32_t av1mi_fg_abs_response(const int *a, const int *b, const int *c) {
  const int r = (a[0] - 2 * a[1] + a[2]) - 2 * (b[0] - 2 * b[1] + b[2]) + (c[0] - 2 * c[1] + c[2]);
  return (uint32_t)(r < 0 ? -r : r);
}
// Nsum of an n x n block (n = 16 luma, 8 chroma) of samples at x[row * stride + column]
template <class T>
AV1MI_FG_HD inline uint32_t av1mi_fg_nsum(const T *x, size_t stride, int n) {
  uint32_t s = 0;
  for (int r = 1; r < n - 1; r++)
    for (int c = 1; c < n - 1; c++) {
      int a[3], b[3], d[3];
      for (int k = 0; k < 3; k++) { a[k] = x[(r - 1) * stride + c - 1 + k]; b[k] = x[r * stride + c - 1 + k]; d[k] = x[(r + 1) * stride + c - 1 + k]; }
      s += av1mi_fg_abs_response(a, b, d);
    }
  return s;
}

// the lower quartile of a histogram of 256 counters holding n > 0 values: the smallest v whose cumulative count reaches (n + 3) / 4
template <class T>
AV1MI_FG_HD inline int av1mi_fg_quartile(const T *hist, uint32_t n) {
  const uint32_t rank = (n + 3) / 4;
  uint32_t cum = 0;
  for (int v = 0; v < 255; v++) {
    cum += hist[v];
    if (cum >= rank) return v;
  }
  return 255;
}
// the value of bin k of a plane: its own if it is populated, else the nearest populated bin's (the lower index on a tie), 0 if there is
// none; count[] and value[] over the plane's eight bins (value[] is read at populated bins only), then the clamp
AV1MI_FG_HD inline int av1mi_fg_fill(const uint32_t *count, const int *value, int k, int ceiling) {
  int v = 0;
  for (int d = 0; d < AV1MI_FG_BINS; d++) {
    if (k - d >= 0 && count[k - d] >= AV1MI_FG_MIN_BLOCKS) { v = value[k - d]; break; }
    if (k + d < AV1MI_FG_BINS && count[k + d] >= AV1MI_FG_MIN_BLOCKS) { v = value[k + d]; break; }
  }
  return v > ceiling ? ceiling : v;
}
// ---- the block walk of fg_block_kernel and fg_ar_sums_kernel: both place their lanes and blocks by these functions alone, so the fit
// visits the estimate's records where the estimate put them (tests/host/fg_rule_host.cpp runs the walk on the CPU).  A workgroup of three
// waves takes four PAIRS of horizontally adjacent blocks a step, eight block slots: waves 0 and 1 are 128 luma lanes, 16 rows of each slot's
// block; wave 2 is 2 x 32 chroma lanes, 8 U (V) rows of each pair - a lane sits at the pair's left slot and holds 2 x 8 samples.
#define AV1MI_FG_WALK_THREADS 192
#define AV1MI_FG_WALK_SLOTS 8
struct Av1miFgLane { bool luma; int slot, row, plane; };   // (luma is wave-uniform)
AV1MI_FG_HD inline Av1miFgLane av1mi_fg_walk_lane(int t) {
  const bool luma = t < 128;
  return { luma, luma ? t >> 4 : ((t >> 3) & 3) * 2, luma ? t & 15 : t & 7, luma ? 0 : 1 + ((t - 128) >> 5) };
}
// the steps of a chunk of n_frames frames of nbx x nby blocks
AV1MI_FG_HD inline long av1mi_fg_walk_steps(int n_frames, int nbx, int nby) { return ((long)n_frames * nby * ((nbx + 1) / 2) + 3) / 4; }
// the block of a slot at a step < av1mi_fg_walk_steps: pair (step * 4 + slot / 2) in frame, row, column order, side slot & 1.  here:
// the block exists (f, by, bx are then inside the chunk); both: so does the block right of it - for a chroma lane, its pair's right half
struct Av1miFgSpot { int f, by, bx; bool here, both; };
AV1MI_FG_HD inline Av1miFgSpot av1mi_fg_walk_spot(long step, int slot, int n_frames, int nbx, int nby) {
  const int npx = (nbx + 1) / 2;
  const long per_frame = (long)nby * npx, gp = step * 4 + (slot >> 1);
  const int in_frame = (int)(gp % per_frame), bx = (in_frame % npx) * 2 + (slot & 1);
  const bool here = gp < n_frames * per_frame && bx < nbx;
  return { (int)(gp / per_frame), in_frame / npx, bx, here, here && bx + 1 < nbx };
}

// writes the 8 bits of v at bit offset `bit` of h (MSB first, like the header's writer)
AV1MI_FG_HD inline void av1mi_fg_put8(uint8_t *h, int bit, uint32_t v) {
  const int i = bit >> 3, sh = bit & 7;
  h[i] = (uint8_t)((h[i] & ~(0xFFu >> sh)) | (v >> sh));
  if (sh) h[i + 1] = (uint8_t)((h[i + 1] & (0xFFu >> sh)) | ((v << (8 - sh)) & 0xFFu));
}

#endif
