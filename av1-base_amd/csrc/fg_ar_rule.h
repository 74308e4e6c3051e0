// fg_ar_rule.h - the film grain's autoregressive coefficients fitted to the chunk's source (av1mi_params.film_grain bits 12-13 with bit 8:
// AV1MI_FILM_GRAIN_AR(lag)), all integers, for host and device: fg_ar_kernel.hip runs it per block and per chunk,
// tests/host/fg_ar_rule_host.cpp compiles it for the CPU against the numpy restatement (tests/fg_ar_ref.py).  Non-normative: the decoder
// only sees ar_coeff_lag, the coefficients and the scaled points of the frame headers.  rdiv is av1mi_fit_rdiv: rounded, halves away from 0.
//
//   flat block   per plane p, from the estimate's record { bin k, v_y, v_u, v_v } and the bins' quartiles q_p[k] before fill and ceiling
//                (fg_rule.h): bin k populated (at least 16 blocks) and q_p[k] >= 1; v_p <= q_p[k]; and sum e^2 <= n^2 (q_p[k] << (bd - 8))^2,
//                16 sigma^2 of what the table says (e is in sixteenths, the table in 64ths of an 8-bit sample).  Immerkaer's operator
//                is blind to f(x) + g(y) - a step edge along an axis has v = 0 - and the third condition keeps those out.  It also
//                bounds everything below: sum e^2 <= 256 * 1020^2 < 2^28 per block, so |e| < 2^14, any sum of products of distinct
//                pairs of a block is at most sum e^2 (|a b| <= (a^2 + b^2) / 2) and fits 32 bits, and a chunk's sums stay below 2^54
//                (8K x 240 frames: 2^26 blocks)
//   noise        n x n samples, n = 16 luma / 8 chroma, less their least-squares plane, exactly: u = 2 c - (n - 1), v = 2 r - (n - 1),
//                S = sum x, A = sum u x, B = sum v x, Q = n sum_c u^2 = 21760 / 1344, Q / n^2 = 85 / 21;
//                e[r][c] = rdiv(16 (Q x - (Q / n^2) S - u A - v B), Q).  |the numerator| <= 16 (2.3e7 + 2 * 15 * 2.1e6) < 1.4e9 < 2^31,
//                so |e| < 2^16 and e^2 fits 32 bits before the block is known to be flat
//   sums         R[dy][dx], dy = 0 .. L, dx = -2 L .. 2 L (dy = 0: dx >= 0): sum of e[r][c] e[r + dy][c + dx] over the flat blocks of every
//                frame and the positions with both samples inside the block; F: the flat blocks.  A plane's 46 sums stand at
//                k = dx (dy = 0, dx = 0 .. 6) and k = 7 + 13 (dy - 1) + dx + 6 (dy = 1 .. 3, dx = -6 .. 6), zeros beyond the lag's reach
//   normalise    rho[d] = clamp(rdiv(R[d] n^2 2^20, R[0] (n - dy) (n - |dx|)), -2^20, 2^20), rho[-d] = rho[d]; the fit is absent if F < 16 or
//                R[0] <= 0.  The numerator reaches 2^82: the product is kept in two 64-bit words and divided bit by bit (av1mi_fgar_muldiv),
//                the denominator is below 2^62
//   solve        positions p_i in the order the spec codes them, rows -L .. 0, columns -L .. L, up to (0, 0): 2 L (L + 1);
//                A[i][j] = rho[p_i - p_j], b[i] = rho[p_i]; A = L D L^T in Q20, rmul(a, b) = rdiv(a b, 2^20), column by column:
//                  w[k] = rmul(L[j][k], d[k]) (k < j);  d[j] = A[j][j] - sum_k rmul(L[j][k], w[k]), absent unless 2^8 <= d[j] <= 2^21;
//                  i > j: t = A[i][j] - sum_k rmul(L[i][k], w[k]), L[i][j] = rdiv(t 2^20, d[j]), absent if |t| or |L[i][j]| > 2^30;
//                then z[i] = b[i] - sum_{k < i} rmul(L[i][k], z[k]), y[i] = rdiv(z[i] 2^20, d[i]), and from the last i down
//                a[i] = y[i] - sum_{k > i} rmul(L[k][i], a[k]); absent if any |z|, |y| or |a| > 2^30.  Every stored operand is at most
//                2^30 (w: 2^31), so a product is below 2^62, a sum of 24 rounded products below 2^47 and t 2^20 below 2^51: 64 bits hold all
//   quantise     c_i = clamp(rdiv(a_i, 2^13), -128, 127): Q7, ar_coeff_shift_minus_6 = 1;
//                E = 2^34 - 2^8 sum c_i b_i + sum_ij c_i c_j A[i][j], the innovation's share of the variance at scale 2^34 (|terms| < 2^45);
//                absent if E <= 0, E > 2^34 or E < 2^30 (a filter that amplifies more than 4 times); g = isqrt(E >> 18), Q8, 64 .. 256;
//                every point of the plane becomes (value g + 128) >> 8, from the value after the ceiling.  Absent: all c_i = 0, g = 256
//   chroma       the luma tap, the last of a chroma plane's 2 L (L + 1) + 1 coefficients, stays 0
#ifndef AV1MI_FG_AR_RULE_H
#define AV1MI_FG_AR_RULE_H
#include "fg_rule.h"
#include "lr_fit_rule.h"

#define AV1MI_FGAR_MAX_LAG 3
#define AV1MI_FGAR_SUMS 46                     /* the sums of one plane */
#define AV1MI_FGAR_PART (AV1MI_FGAR_SUMS + 1)  /* ... and its count of flat blocks: what a workgroup stores per plane */
#define AV1MI_FGAR_MAX_POS 24                  /* 2 L (L + 1) at L = 3 */
#define AV1MI_FGAR_COEFFS 25                   /* coefficients reported per plane: the positions, and chroma's luma tap */
#define AV1MI_FGAR_MIN_FLAT 16
#define AV1MI_FGAR_ONE (1ll << 20)
#define AV1MI_FGAR_LIMIT (1ll << 30)
#define AV1MI_FGAR_WS (AV1MI_FGAR_MAX_POS * AV1MI_FGAR_MAX_POS + 4 * AV1MI_FGAR_MAX_POS)   /* 64-bit words av1mi_fgar_solve works in */

// the positions of lag L, and the film_grain_params bits it adds to the estimate's (three planes' coefficients of 8 bits)
AV1MI_FG_HD inline int av1mi_fgar_positions(int lag) { return 2 * lag * (lag + 1); }
AV1MI_FG_HD inline int av1mi_fgar_extra_bits(int lag) { return 48 * lag * (lag + 1); }
// Q and Q / n^2 of a block of n x n
AV1MI_FG_HD inline int av1mi_fgar_q(int n) { return n == 16 ? 21760 : 1344; }
AV1MI_FG_HD inline int av1mi_fgar_qn(int n) { return n == 16 ? 85 : 21; }

// e of the sample x at row r, column c of an n x n block with the sums S, A, B
AV1MI_FG_HD inline int av1mi_fgar_residual(int n, int x, int r, int c, int S, int A, int B) {
  const int Q = av1mi_fgar_q(n), u = 2 * c - (n - 1), v = 2 * r - (n - 1);
  const int a = 16 * (Q * x - av1mi_fgar_qn(n) * S - u * A - v * B);
  const int q = (int)(((uint32_t)(a < 0 ? -a : a) + (uint32_t)(Q >> 1)) / (uint32_t)Q);
  return a < 0 ? -q : q;
}
// the third condition of a flat block: the block's sum of e^2 against the bin's quartile q
AV1MI_FG_HD inline bool av1mi_fgar_energy_ok(uint64_t energy, int n, int q, int bit_depth) {
  const uint64_t s = (uint64_t)q << (bit_depth - 8);
  return energy <= (uint64_t)(n * n) * s * s;
}
// the first two: record r, plane pl, the plane's quartiles and counts over its eight bins
AV1MI_FG_HD inline bool av1mi_fgar_candidate(uint32_t rec, int pl, const int *quart, const uint32_t *count) {
  const int k = (int)(rec & 7u), v = (int)((rec >> (8 + 8 * pl)) & 0xFFu);
  return count[k] >= AV1MI_FG_MIN_BLOCKS && quart[k] >= 1 && v <= quart[k];
}

// where R[dy][dx] stands among a plane's sums (dy = 0 .. 3; dx = 0 .. 6 for dy = 0, else -6 .. 6), and the reverse
AV1MI_FG_HD inline int av1mi_fgar_index(int dy, int dx) { return dy == 0 ? dx : 7 + 13 * (dy - 1) + dx + 6; }
AV1MI_FG_HD inline int av1mi_fgar_index_dy(int k) { return k < 7 ? 0 : 1 + (k - 7) / 13; }
AV1MI_FG_HD inline int av1mi_fgar_index_dx(int k) { return k < 7 ? k : (k - 7) % 13 - 6; }
AV1MI_FG_HD inline bool av1mi_fgar_index_used(int k, int lag) {
  const int dy = av1mi_fgar_index_dy(k), dx = av1mi_fgar_index_dx(k);
  return dy <= lag && (dx < 0 ? -dx : dx) <= 2 * lag;
}

// the sums of an n x n block of residuals e[r * n + c] added to R (reference form: the kernel forms the same sums row by row)
AV1MI_FG_HD inline void av1mi_fgar_block_sums(const int *e, int n, int lag, long long *R) {
  for (int k = 0; k < AV1MI_FGAR_SUMS; k++) {
    if (!av1mi_fgar_index_used(k, lag)) continue;
    const int dy = av1mi_fgar_index_dy(k), dx = av1mi_fgar_index_dx(k);
    long long s = 0;
    for (int r = 0; r + dy < n; r++)
      for (int c = dx < 0 ? -dx : 0; c < n && c + dx < n; c++) s += (long long)e[r * n + c] * e[(r + dy) * n + c + dx];
    R[k] += s;
  }
}
// the residuals of a block of samples x[row * stride + column] into e[n * n]; returns the sum of their squares
template <class T>
AV1MI_FG_HD inline uint64_t av1mi_fgar_block_noise(const T *x, size_t stride, int n, int *e) {
  int S = 0, A = 0, B = 0;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) { const int s = x[r * stride + c]; S += s; A += (2 * c - (n - 1)) * s; B += (2 * r - (n - 1)) * s; }
  uint64_t en = 0;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) {
      const int v = av1mi_fgar_residual(n, x[r * stride + c], r, c, S, A, B);
      e[r * n + c] = v;
      en += (uint64_t)((long long)v * v);
    }
  return en;
}

// min(limit, rdiv(|a| m, den)) with the sign of a: |a| < 2^62, m <= 2^28, 0 < den < 2^62.  The product in two words, the quotient bit by bit
AV1MI_FG_HD inline long long av1mi_fgar_muldiv(long long a, uint32_t m, uint64_t den, long long limit) {
  const uint64_t ua = (uint64_t)(a < 0 ? -a : a);
  const uint64_t p0 = (ua & 0xFFFFFFFFull) * m, p1 = (ua >> 32) * m;   // < 2^60, < 2^58
  uint64_t lo = p0 + (p1 << 32), hi = (p1 >> 32) + (lo < p0 ? 1 : 0);
  const uint64_t half = den >> 1;
  lo += half;
  hi += lo < half ? 1 : 0;
  uint64_t rem = 0, q = 0;
  bool sat = false;
  for (int i = 127; i >= 0; i--) {
    const uint64_t bit = i >= 64 ? (hi >> (i - 64)) & 1u : (lo >> i) & 1u;
    rem = (rem << 1) | bit;   // (rem < den before: below 2^63 after)
    if (q >> 62) sat = true;
    q = sat ? q : q << 1;
    if (rem >= den) { rem -= den; q |= 1u; }
  }
  const long long r = sat || q > (uint64_t)limit ? limit : (long long)q;
  return a < 0 ? -r : r;
}
// rho at index k of a plane's sums R for blocks of n x n (R[0] > 0)
AV1MI_FG_HD inline int av1mi_fgar_rho(const long long *R, int k, int n) {
  const int dy = av1mi_fgar_index_dy(k), dx = av1mi_fgar_index_dx(k);
  const uint64_t den = (uint64_t)R[0] * (uint64_t)((n - dy) * (n - (dx < 0 ? -dx : dx)));
  return (int)av1mi_fgar_muldiv(R[k], (uint32_t)(n * n) << 20, den, AV1MI_FGAR_ONE);
}
AV1MI_FG_HD inline long long av1mi_fgar_rho_at(const int *rho, int dy, int dx) {
  if (dy < 0 || (dy == 0 && dx < 0)) { dy = -dy; dx = -dx; }
  return rho[av1mi_fgar_index(dy, dx)];
}
// position i of lag L: row -L .. 0, column -L .. L
AV1MI_FG_HD inline int av1mi_fgar_pos_row(int i, int lag) { return i / (2 * lag + 1) - lag; }
AV1MI_FG_HD inline int av1mi_fgar_pos_col(int i, int lag) { return i % (2 * lag + 1) - lag; }
AV1MI_FG_HD inline long long av1mi_fgar_a_at(const int *rho, int lag, int i, int j) {
  return av1mi_fgar_rho_at(rho, av1mi_fgar_pos_row(i, lag) - av1mi_fgar_pos_row(j, lag), av1mi_fgar_pos_col(i, lag) - av1mi_fgar_pos_col(j, lag));
}
AV1MI_FG_HD inline long long av1mi_fgar_b_at(const int *rho, int lag, int i) { return av1mi_fgar_rho_at(rho, av1mi_fgar_pos_row(i, lag), av1mi_fgar_pos_col(i, lag)); }
AV1MI_FG_HD inline long long av1mi_fgar_rmul(long long a, long long b) { return av1mi_fit_rdiv(a * b, AV1MI_FGAR_ONE); }
AV1MI_FG_HD inline bool av1mi_fgar_within(long long v) { return v >= -AV1MI_FGAR_LIMIT && v <= AV1MI_FGAR_LIMIT; }

// the coefficients a[2 L (L + 1)] in Q20 from rho (a plane's 46 values); ws: AV1MI_FGAR_WS words to work in.  Returns 0 if the fit is absent
AV1MI_FG_HD inline int av1mi_fgar_solve(int lag, const int *rho, long long *ws, long long *a) {
  const int N = av1mi_fgar_positions(lag), M = AV1MI_FGAR_MAX_POS;
  long long *L = ws, *d = ws + M * M, *w = d + M, *z = w + M, *y = z + M;
  for (int j = 0; j < N; j++) {
    for (int k = 0; k < j; k++) w[k] = av1mi_fgar_rmul(L[j * M + k], d[k]);
    long long t = av1mi_fgar_a_at(rho, lag, j, j);
    for (int k = 0; k < j; k++) t -= av1mi_fgar_rmul(L[j * M + k], w[k]);
    if (t < (1 << 8) || t > (1 << 21)) return 0;
    d[j] = t;
    for (int i = j + 1; i < N; i++) {
      t = av1mi_fgar_a_at(rho, lag, i, j);
      for (int k = 0; k < j; k++) t -= av1mi_fgar_rmul(L[i * M + k], w[k]);
      if (!av1mi_fgar_within(t)) return 0;
      const long long l = av1mi_fit_rdiv(t * AV1MI_FGAR_ONE, d[j]);
      if (!av1mi_fgar_within(l)) return 0;
      L[i * M + j] = l;
    }
  }
  for (int i = 0; i < N; i++) {
    long long t = av1mi_fgar_b_at(rho, lag, i);
    for (int k = 0; k < i; k++) t -= av1mi_fgar_rmul(L[i * M + k], z[k]);
    if (!av1mi_fgar_within(t)) return 0;
    z[i] = t;
    y[i] = av1mi_fit_rdiv(t * AV1MI_FGAR_ONE, d[i]);
    if (!av1mi_fgar_within(y[i])) return 0;
  }
  for (int i = N - 1; i >= 0; i--) {
    long long t = y[i];
    for (int k = i + 1; k < N; k++) t -= av1mi_fgar_rmul(L[k * M + i], a[k]);
    if (!av1mi_fgar_within(t)) return 0;
    a[i] = t;
  }
  return 1;
}

AV1MI_FG_HD inline uint32_t av1mi_fgar_isqrt(uint32_t v) {   // floor(sqrt(v)), v <= 2^16
  uint32_t r = 0;
  for (uint32_t b = 1u << 8; b; b >>= 1) if ((r + b) * (r + b) <= v) r += b;
  return r;
}
// the Q7 coefficients c[2 L (L + 1)] and the gain from a[]; returns 0 - the fit is absent after all - with c all 0 and the gain 256
AV1MI_FG_HD inline int av1mi_fgar_quantise(int lag, const int *rho, const long long *a, int8_t *c, uint32_t *gain) {
  const int N = av1mi_fgar_positions(lag);
  for (int i = 0; i < N; i++) c[i] = (int8_t)av1mi_fit_clamp(av1mi_fit_rdiv(a[i], 1 << 13), -128, 127);
  long long E = 1ll << 34;
  for (int i = 0; i < N; i++) {
    E -= 256 * (long long)c[i] * av1mi_fgar_b_at(rho, lag, i);
    for (int j = 0; j < N; j++) E += (long long)c[i] * c[j] * av1mi_fgar_a_at(rho, lag, i, j);
  }
  if (E <= 0 || E > (1ll << 34) || E < (1ll << 30)) {
    for (int i = 0; i < N; i++) c[i] = 0;
    *gain = 256;
    return 0;
  }
  *gain = av1mi_fgar_isqrt((uint32_t)(E >> 18));
  return 1;
}
// steps 4 - 6 of a plane: its sums R, flat blocks F, block size n; c[AV1MI_FGAR_COEFFS] (the luma tap and what the lag does not use: 0), the
// gain; rho: 46 words and ws: AV1MI_FGAR_WS words to work in (rho[] must hold av1mi_fgar_rho of every used index when `have_rho`).
// Returns whether the fit is present
AV1MI_FG_HD inline int av1mi_fgar_fit(int lag, const long long *R, uint32_t F, int n, int *rho, bool have_rho, long long *ws, int8_t *c, uint32_t *gain) {
  for (int i = 0; i < AV1MI_FGAR_COEFFS; i++) c[i] = 0;
  *gain = 256;
  if (F < AV1MI_FGAR_MIN_FLAT || R[0] <= 0) return 0;
  if (!have_rho)
    for (int k = 0; k < AV1MI_FGAR_SUMS; k++) rho[k] = av1mi_fgar_index_used(k, lag) ? av1mi_fgar_rho(R, k, n) : 0;
  long long a[AV1MI_FGAR_MAX_POS];
  if (!av1mi_fgar_solve(lag, rho, ws, a)) return 0;
  return av1mi_fgar_quantise(lag, rho, a, c, gain);
}
AV1MI_FG_HD inline int av1mi_fgar_compensate(int value, uint32_t gain) { return (int)(((uint32_t)value * gain + 128u) >> 8); }

#endif
