// cdef_pieces.h - the pieces of CDEF (spec §7.15) that more than one place needs, compiled for the device and for the host: the
// direction search, the strength rules, the tap geometry with its "not available" rule, the sample filter, what the strength search
//  computes of a sample, and the search's candidate pool.  cdef_sb_kernel and cdef_search_kernel
// (cdef_kernel.hip) both filter through these, so the search scores exactly what the filter will do; tests/host/cdef_pieces_host.cpp
// runs them on the CPU against oracle/av1o_cdef.c.
#ifndef AV1MI_CDEF_PIECES_H
#define AV1MI_CDEF_PIECES_H
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define AV1MI_CDEF_INLINE __host__ __device__ __forceinline__
#else
#define AV1MI_CDEF_INLINE inline
#endif

AV1MI_CDEF_INLINE int av1mi_cdef_iabs(int v) { return v < 0 ? -v : v; }
AV1MI_CDEF_INLINE int av1mi_cdef_constrain(int diff, int threshold, int shift) {
  // shift = av1mi_cdef_damp_shift(threshold, damping), precomputed by the caller; threshold 0 gives 0
  const int mag = av1mi_cdef_iabs(diff);
  int lim = threshold - (mag >> shift);
  lim = lim < 0 ? 0 : (lim > mag ? mag : lim);
  return diff < 0 ? -lim : lim;
}
// max(0, damping - floor(log2(threshold)))
AV1MI_CDEF_INLINE int av1mi_cdef_damp_shift(int threshold, int damping) {
  if (!threshold) return 0;
  const int a = damping - (31 - __builtin_clz((unsigned)threshold));
  return a < 0 ? 0 : a;
}

// Cdef_Directions[d][k] = (dy, dx), packed 3 bits per direction (value + 2) so that the tap offsets cost
// a shift and a mask instead of a dependent table load per tap.
AV1MI_CDEF_INLINE void av1mi_cdef_dir_offsets(int dir, int &dy0, int &dx0, int &dy1, int &dx1) {
  //            d: 7  6  5  4  3  2  1  0
  // k=0 dy+2:     3  3  3  3  2  2  2  1      dx+2: 2 2 2 3 3 3 3 3
  // k=1 dy+2:     4  4  4  4  3  2  1  0      dx+2: 1 2 3 4 4 4 4 4
  const int sh = 3 * dir;
  dy0 = ((0x6DB491 >> sh) & 7) - 2;   // 011 011 011 011 010 010 010 001
  dx0 = ((0x4936DB >> sh) & 7) - 2;   // 010 010 010 011 011 011 011 011
  dy1 = ((0x924688 >> sh) & 7) - 2;   // 100 100 100 100 011 010 001 000
  dx1 = ((0x29C924 >> sh) & 7) - 2;   // 001 010 011 100 100 100 100 100
}
// The taps of a sample filtered along `dir`, as offsets (ty, tx), in the one order every user keeps: k = 0 .. 3 primary (distance 1 with
// both signs, then distance 2), NT = 12: k = 4 .. 7 the secondary direction dir + 2 likewise, k = 8 .. 11 dir + 6.  Taps k and k ^ 1 are
// the two signs of one offset.
template <int NT>
AV1MI_CDEF_INLINE void av1mi_cdef_tap_offsets(int dir, int (&ty)[NT], int (&tx)[NT]) {
  static_assert(NT == 4 || NT == 12, "primary taps, or primary and secondary");
#pragma unroll
  for (int g = 0; g < NT / 4; g++) {
    int dy[2], dx[2];
    av1mi_cdef_dir_offsets(g == 0 ? dir : (dir + (g == 1 ? 2 : 6)) & 7, dy[0], dx[0], dy[1], dx[1]);
#pragma unroll
    for (int k = 0; k < 2; k++) { ty[4 * g + 2 * k] = dy[k]; tx[4 * g + 2 * k] = dx[k]; ty[4 * g + 2 * k + 1] = -dy[k]; tx[4 * g + 2 * k + 1] = -dx[k]; }
  }
}
// weight of tap k in that order.  odd: bit 0 of the primary strength at 8-bit scale, (pri >> coeff_shift) & 1
// taps k = 0, 1: primary, distance 1 (weight 4 or 3); 2, 3: primary, distance 2 (2 or 3); 4 .. 11: secondary (2, 2, 1, 1 per direction)
AV1MI_CDEF_INLINE int av1mi_cdef_tap_weight(int k, int odd) { return k < 2 ? (odd ? 3 : 4) : (k < 4 ? (odd ? 3 : 2) : (((k - 4) & 3) < 2 ? 2 : 1)); }

// "Not available" (§7.15.3): a tap outside the frame counts as the centre sample x, which contributes nothing to the sum nor to
// the clamp range.  av1mi_cdef_tap_pos: is the tap of (gy, gx) at offset (dy, dx) inside the w x h plane?  (yy, xx): its position
// clamped into the plane, which can always be loaded.
AV1MI_CDEF_INLINE bool av1mi_cdef_tap_pos(int gy, int gx, int dy, int dx, int w, int h, int *yy, int *xx) {
  const int y = gy + dy, x = gx + dx;
  *yy = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
  *xx = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
  return y >= 0 && x >= 0 && y < h && x < w;
}
AV1MI_CDEF_INLINE int av1mi_cdef_tap_or_centre(bool ok, int tap, int x) { return ok ? tap : x; }
// sample `idx` of a plane: the byte offset is formed in 32 bits (a frame is far below 4 GB), so a device load takes its address as
// scalar base + 32-bit vector offset
template <typename PIX>
AV1MI_CDEF_INLINE int av1mi_cdef_ld(const PIX *pl, int idx) {
  return *reinterpret_cast<const PIX *>(reinterpret_cast<const char *>(pl) + (unsigned)idx * (unsigned)sizeof(PIX));
}
// one tap's value.  EDGE = false: the caller knows that every tap is inside (interior superblocks)
template <typename PIX, bool EDGE>
AV1MI_CDEF_INLINE int av1mi_cdef_tap(const PIX *pl, int stride, int w, int h, int gy, int gx, int dy, int dx, int x) {
  if (!EDGE) return av1mi_cdef_ld(pl, (gy + dy) * stride + gx + dx);
  int yy, xx;
  if (!av1mi_cdef_tap_pos(gy, gx, dy, dx, w, h, &yy, &xx)) return x;
  return av1mi_cdef_ld(pl, yy * stride + xx);
}

// ---- the sample filter (§7.15.3)
// the finish: the weighted sum rounded into the sample, clamped to the range of the sample and its taps
AV1MI_CDEF_INLINE int av1mi_cdef_round(int x, int sum) { return x + ((8 + sum - (sum < 0)) >> 4); }
AV1MI_CDEF_INLINE int av1mi_cdef_finish(int x, int sum, int mn, int mx) {
  const int v = av1mi_cdef_round(x, sum);
  return v < mn ? mn : (v > mx ? mx : v);
}
// centre x and its NT loaded taps t[] in av1mi_cdef_tap_offsets' order; okm: bit k = tap k is available (~0u: all).  Strength 0 on both
// gives x itself.
template <int NT>
AV1MI_CDEF_INLINE int av1mi_cdef_sample(int x, const int (&t)[NT], unsigned okm, int pri, int pri_shift, int sec, int sec_shift, int odd) {
  int sum = 0, mx = x, mn = x;
#pragma unroll
  for (int k = 0; k < NT; k++) {
    const int p = av1mi_cdef_tap_or_centre((okm >> k) & 1, t[k], x);
    sum += av1mi_cdef_tap_weight(k, odd) * (k < 4 ? av1mi_cdef_constrain(p - x, pri, pri_shift) : av1mi_cdef_constrain(p - x, sec, sec_shift));
    mx = p > mx ? p : mx;
    mn = p < mn ? p : mn;
  }
  return av1mi_cdef_finish(x, sum, mn, mx);
}

// ---- direction search §7.15.2 of one 8x8 block held in registers (px[i][j], already >> coeff_shift and - 128): direction and the
// variance that scales the luma primary strength.  The eight directions' partial sums would need 120 registers at once; they
// are built in two groups of four, which keeps the callers at 6 waves/SIMD without spilling.
AV1MI_CDEF_INLINE int av1mi_cdef_div(int n) { return 840 / n; }   // Div_Table[n], n = 1 .. 8: a constant wherever n is one
AV1MI_CDEF_INLINE void av1mi_cdef_direction_8x8(const int (&px)[8][8], int &ydir, int &var) {
  int cost[8];
#pragma unroll
  for (int a = 0; a < 8; a++) cost[a] = 0;
#pragma unroll
  for (int grp = 0; grp < 2; grp++) {
    int partial[4][15];
#pragma unroll
    for (int a = 0; a < 4; a++) {
#pragma unroll
      for (int b = 0; b < 15; b++) partial[a][b] = 0;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int x = px[i][j];
        if (grp == 0) {
          partial[0][i + j] += x;            // direction 0
          partial[1][i + j / 2] += x;        // 1
          partial[2][i] += x;                // 2
          partial[3][3 + i - j / 2] += x;    // 3
        } else {
          partial[0][7 + i - j] += x;        // 4
          partial[1][3 - i / 2 + j] += x;    // 5
          partial[2][j] += x;                // 6
          partial[3][i / 2 + j] += x;        // 7
        }
      }
    }
    const int d0 = grp * 4;
    {  // directions 2 and 6: 8 sums
      int c = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) c += partial[2][i] * partial[2][i];
      cost[d0 + 2] = c * av1mi_cdef_div(8);
    }
    {  // directions 0 and 4: 15 diagonals
      int c = 0;
#pragma unroll
      for (int i = 0; i < 7; i++) c += (partial[0][i] * partial[0][i] + partial[0][14 - i] * partial[0][14 - i]) * av1mi_cdef_div(i + 1);
      cost[d0] = c + partial[0][7] * partial[0][7] * av1mi_cdef_div(8);
    }
#pragma unroll
    for (int q = 1; q < 4; q += 2) {  // odd directions: 11 sums
      int c = 0;
#pragma unroll
      for (int j = 0; j < 5; j++) c += partial[q][3 + j] * partial[q][3 + j];
      c *= av1mi_cdef_div(8);
#pragma unroll
      for (int j = 0; j < 3; j++) c += (partial[q][j] * partial[q][j] + partial[q][10 - j] * partial[q][10 - j]) * av1mi_cdef_div(2 * j + 2);
      cost[d0 + q] = c;
    }
  }
  int best = 0;
  ydir = 0;
#pragma unroll
  for (int d = 0; d < 8; d++)
    if (cost[d] > best) { best = cost[d]; ydir = d; }
  int opp = 0;
#pragma unroll
  for (int d = 0; d < 8; d++)
    if (d == ((ydir + 4) & 7)) opp = cost[d];
  var = (best - opp) >> 10;
}
// the block's samples as the direction search takes them
template <typename PIX>
AV1MI_CDEF_INLINE void av1mi_cdef_block_direction(const PIX *blk8, int stride, int coeff_shift, int &ydir, int &var) {
  int px[8][8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) px[i][j] = ((int)blk8[(size_t)i * stride + j] >> coeff_shift) - 128;
  }
  av1mi_cdef_direction_8x8(px, ydir, var);
}

// ---- strengths (§7.15.1).  y_pri, uv_pri, *_sec: the header's fields; a secondary field of 3 means strength 4
AV1MI_CDEF_INLINE int av1mi_cdef_sec_strength(int sec_field, int coeff_shift) { return (sec_field == 3 ? 4 : sec_field) << coeff_shift; }
// variance-adjusted luma primary strength
AV1MI_CDEF_INLINE int av1mi_cdef_adjusted_pri(int pri_y, int var, int coeff_shift) {
  int pri = pri_y << coeff_shift;
  const int v6 = var >> 6;
  const int var_str = v6 ? ((31 - __builtin_clz((unsigned)v6)) < 12 ? (31 - __builtin_clz((unsigned)v6)) : 12) : 0;
  return var ? (pri * (4 + var_str) + 8) >> 4 : 0;
}

// ---- the candidate pool of the strength search: primary strength P8[i] = 0, 1, 2, 3, 4, 6, 8, 11 as nibbles.  Luma
// candidate l = 0 .. 15 is (P8[l >> 1], secondary code 2 * (l & 1)), chroma candidate c = 0 .. 7 is (P8[c], 0); pair p = 8 l + c.
AV1MI_CDEF_INLINE int av1mi_cdef_pool_pri(int i) { return (int)((0xB8643210u >> (4 * i)) & 15u); }
struct Av1miCdefStrengths { int y_pri, y_sec, uv_pri, uv_sec; };   // the header's four fields
AV1MI_CDEF_INLINE Av1miCdefStrengths av1mi_cdef_pair_strengths(int p) {
  const int l = p >> 3, c = p & 7;
  return { av1mi_cdef_pool_pri(l >> 1), (l & 1) * 2, av1mi_cdef_pool_pri(c), 0 };
}
// cdef_y_pri_strength (4 bits), cdef_y_sec_strength (2), cdef_uv_pri_strength (4), cdef_uv_sec_strength (2), MSB first
AV1MI_CDEF_INLINE uint32_t av1mi_cdef_pair_bits(int p) {
  const Av1miCdefStrengths s = av1mi_cdef_pair_strengths(p);
  return ((uint32_t)s.y_pri << 8) | ((uint32_t)s.y_sec << 6) | ((uint32_t)s.uv_pri << 2) | (uint32_t)s.uv_sec;
}
// a superblock's error under pair p, from its 16 luma and 8 chroma (U + V) candidate errors e[24]
AV1MI_CDEF_INLINE int av1mi_cdef_pair_luma_at(int p) { return p >> 3; }           // where in e[24] the pair's luma candidate stands
AV1MI_CDEF_INLINE int av1mi_cdef_pair_chroma_at(int p) { return 16 + (p & 7); }   // ... and its chroma candidate
AV1MI_CDEF_INLINE unsigned long long av1mi_cdef_pair_err(const unsigned long long *e, int p) { return e[av1mi_cdef_pair_luma_at(p)] + e[av1mi_cdef_pair_chroma_at(p)]; }

// ---- what the search computes of one sample x at (gy, gx): the filter's output under every candidate.  The taps are loaded once and their
// range and secondary sum formed once; only the strength-dependent part of constrain() runs per candidate.
//   luma  l = 0: the sample itself; l = 1 (primary 0, secondary 2): the sample filter on direction 0's taps (a zero primary strength
//         selects direction 0, §7.15.1); l = 2 j (primary P8[j], variance-adjusted per block): the 4 primary taps of the block's direction;
//         l = 2 j + 1: the same primary sum plus the secondary sum of that direction, which all seven share, clamped to its 12 taps.
//   chroma c = 0: the sample itself; c = 1 .. 7: 4 primary taps (P8[c], not variance-adjusted).
// A sum of primary taps alone never leaves the range of its taps (the weights total 12 < 16), so the primary-only candidates are
// rounded and not clamped.
// sum over taps [K0, K1) of weight x constrained difference (taps k, k + 1: one weight)
template <int K0, int K1, int NT>
AV1MI_CDEF_INLINE int av1mi_cdef_tap_sum(int x, const int (&t)[NT], int strength, int shift, int odd) {
  int sum = 0;
#pragma unroll
  for (int k = K0; k < K1; k += 2)
    sum += av1mi_cdef_tap_weight(k, odd) * (av1mi_cdef_constrain(t[k] - x, strength, shift) + av1mi_cdef_constrain(t[k + 1] - x, strength, shift));
  return sum;
}
template <typename PIX, bool EDGE, int NT>
AV1MI_CDEF_INLINE void av1mi_cdef_load_taps(const PIX *pl, int stride, int w, int h, int gy, int gx, int dir, int x, int (&t)[NT]) {
  int ty[NT], tx[NT];
  av1mi_cdef_tap_offsets<NT>(dir, ty, tx);
#pragma unroll
  for (int k = 0; k < NT; k++) t[k] = av1mi_cdef_tap<PIX, EDGE>(pl, stride, w, h, gy, gx, ty[k], tx[k], x);
}
// damping: the luma damping at the samples' scale, cdef_damping + coeff_shift
template <typename PIX, bool EDGE>
AV1MI_CDEF_INLINE void av1mi_cdef_search_luma(const PIX *pl, int stride, int w, int h, int gy, int gx, int x, int dir, int var, int coeff_shift,
                                              int damping, int (&v)[16]) {
  const int sec = av1mi_cdef_sec_strength(2, coeff_shift), sec_shift = av1mi_cdef_damp_shift(sec, damping);
  int t[12];
  av1mi_cdef_load_taps<PIX, EDGE, 12>(pl, stride, w, h, gy, gx, dir, x, t);
  int mx = x, mn = x;
#pragma unroll
  for (int k = 0; k < 12; k++) { mx = t[k] > mx ? t[k] : mx; mn = t[k] < mn ? t[k] : mn; }
  const int ssum = av1mi_cdef_tap_sum<4, 12>(x, t, sec, sec_shift, 0);
  v[0] = x;
  if (dir == 0) {
    v[1] = av1mi_cdef_finish(x, ssum, mn, mx);
  } else {
    int t0[12];
    av1mi_cdef_load_taps<PIX, EDGE, 12>(pl, stride, w, h, gy, gx, 0, x, t0);
    v[1] = av1mi_cdef_sample<12>(x, t0, ~0u, 0, 0, sec, sec_shift, 0);
  }
#pragma unroll
  for (int j = 1; j < 8; j++) {
    const int pri = av1mi_cdef_adjusted_pri(av1mi_cdef_pool_pri(j), var, coeff_shift);
    const int psum = av1mi_cdef_tap_sum<0, 4>(x, t, pri, av1mi_cdef_damp_shift(pri, damping), (pri >> coeff_shift) & 1);
    v[2 * j] = av1mi_cdef_round(x, psum);
    v[2 * j + 1] = av1mi_cdef_finish(x, psum + ssum, mn, mx);
  }
}
// damping: the chroma damping at the samples' scale, cdef_damping + coeff_shift - 1
template <typename PIX, bool EDGE>
AV1MI_CDEF_INLINE void av1mi_cdef_search_chroma(const PIX *pl, int stride, int w, int h, int gy, int gx, int x, int dir, int coeff_shift, int damping,
                                                int (&v)[8]) {
  int t[4];
  av1mi_cdef_load_taps<PIX, EDGE, 4>(pl, stride, w, h, gy, gx, dir, x, t);
  v[0] = x;
#pragma unroll
  for (int c = 1; c < 8; c++) {
    const int pri = av1mi_cdef_pool_pri(c) << coeff_shift;
    v[c] = av1mi_cdef_round(x, av1mi_cdef_tap_sum<0, 4>(x, t, pri, av1mi_cdef_damp_shift(pri, damping), (pri >> coeff_shift) & 1));
  }
}

#endif
