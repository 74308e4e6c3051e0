// wiener_fit_rule.h - the Wiener restoration fit (av1mi_params.enable_lr bit 10, AV1MI_LR_WIENER_FIT), all
// integers, for host and device: lr_wfit_kernel.hip runs it per restoration unit, tests/host/wiener_fit_rule_host.cpp compiles it for
// the CPU against the numpy restatement (tests/wiener_fit_ref.py).  Non-normative except for the syntax: the decoder sees the six
// taps (§5.11.58).
//
//   sample       W = the filter's input (§7.17.6), X its centre, e = src - X; tap k = 0, 1, 2 has the offset o = 3 - k:
//                Dv_k = W[y-o][x] + W[y+o][x] - 2 X,  Dh_k = W[y][x-o] + W[y][x+o] - 2 X
//                (the taps sum to 128: the output is X + (sum a_k Dv_k + sum b_k Dh_k) / 128 + a second-order term the rule drops)
//   unit         27 exact sums: Hvv[j][k] = sum Dv_j Dv_k (00 01 02 11 12 22), Hhh likewise, Hvh[j][k] = sum Dv_j Dh_k
//                (row j), Cv[j] = sum Dv_j e, Ch[k] = sum Dh_k e.  |sum| < 2^40: at 10 bit |D| <= 2 * 1023 < 2^11 and |e| <= 1023, a
//                product is below 2^22, and the largest unit, of 256, has at most 383 x 391 = 149753 < 2^17.2 samples: below 2^39.2
//                (units of 64: at most 95 x 103 samples, below 2^35.3; the edge matrix of tests/lr_edge_cases.py reaches 2^37.06)
//   solve_idx    over a subset of the taps: m = the largest |H[i][j]|, |R[i]| of the subset, s = max(0, bitlength(m) - 17), every
//                entry >> s (arithmetic), Cramer's rule; absent if det <= 0, else x_q = rdiv(128 d_q, det)
//                (after the shift |entry| <= 2^17, a product of three is at most 2^51, a determinant's six at most 6 * 2^51 < 2^53.6,
//                times 128: below 2^60.6, so below 2^62.  Before the shift the refit's and the second stage's sums of H t / Hvh cv
//                hold at most three terms of 2^39.2 * 46: below 2^46.4)
//   solve        x over the taps first .. 2 (first = 1 for chroma: tap 0 is 0 and not coded); t_i = clamp(x_i, Min_i, Max_i); if the
//                clamp acted on some taps but not on all, the free ones are refitted once with the clamped ones held:
//                R2_i = R_i - rdiv(sum_{j clamped} H[i][j] t_j, 128), y = solve_idx(H, R2, free), t_i = clamp(y_i) if y is present
//   two stages   cv = solve(Hvv, Cv);  ch = solve(Hhh, R), R[k] = Ch[k] - rdiv(sum_j Hvh[j][k] cv_j, 128); absent if either is
#ifndef AV1MI_WIENER_FIT_RULE_H
#define AV1MI_WIENER_FIT_RULE_H
#include "lr_fit_rule.h"   // rdiv, clamp, the bit string and lr_put_signed_ref

#define AV1MI_LR_WFIT_SUMS 27
#define AV1MI_LR_WFIT_CHOICE 23   /* a unit's choice when it takes the fitted Wiener filter (0 .. 22: lr_fit_rule.h) */
// offsets into a unit's sums
#define AV1MI_WF_HVV 0
#define AV1MI_WF_HHH 6
#define AV1MI_WF_HVH 12
#define AV1MI_WF_CV 21
#define AV1MI_WF_CH 24

AV1MI_FIT_HD inline int av1mi_wiener_tap_min(int j) { return j == 0 ? -5 : (j == 1 ? -23 : -17); }   // Wiener_Taps_Min
AV1MI_FIT_HD inline int av1mi_wiener_tap_max(int j) { return j == 0 ? 10 : (j == 1 ? 8 : 46); }      // Wiener_Taps_Max
AV1MI_FIT_HD inline int av1mi_wiener_tap_mid(int j) { return j == 0 ? 3 : (j == 1 ? -7 : 15); }      // Wiener_Taps_Mid
// index of (j, k) in a symmetric matrix stored as 00 01 02 11 12 22
AV1MI_FIT_HD inline int av1mi_wf_sym(int j, int k) { const int a = j < k ? j : k, b = j < k ? k : j; return a == 0 ? b : (a == 1 ? 2 + b : 5); }

// x[q] for the taps q of `mask` (bit q; one to three taps) from the full 3 x 3 system; returns 0 if absent
AV1MI_FIT_HD inline int av1mi_wf_solve_idx(const long long H[3][3], const long long R[3], int mask, long long x[3]) {
  int id[3], n = 0;
  for (int q = 0; q < 3; q++) if ((mask >> q) & 1) id[n++] = q;
  unsigned long long m = 0;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) { const long long v = H[id[i]][id[j]]; const unsigned long long a = (unsigned long long)(v < 0 ? -v : v); m = a > m ? a : m; }
    const long long v = R[id[i]]; const unsigned long long a = (unsigned long long)(v < 0 ? -v : v); m = a > m ? a : m;
  }
  int bl = 0;
  while (bl < 64 && (m >> bl)) bl++;
  const int s = bl > 17 ? bl - 17 : 0;
  long long a[3][3], r[3];
  for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) a[i][j] = H[id[i]][id[j]] >> s; r[i] = R[id[i]] >> s; }
  long long det, d[3];
  if (n == 1) { det = a[0][0]; d[0] = r[0]; }
  else if (n == 2) {
    det = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    d[0] = r[0] * a[1][1] - a[0][1] * r[1];
    d[1] = a[0][0] * r[1] - r[0] * a[1][0];
  } else {
    det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    d[0] = r[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (r[1] * a[2][2] - a[1][2] * r[2]) + a[0][2] * (r[1] * a[2][1] - a[1][1] * r[2]);
    d[1] = a[0][0] * (r[1] * a[2][2] - a[1][2] * r[2]) - r[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * r[2] - r[1] * a[2][0]);
    d[2] = a[0][0] * (a[1][1] * r[2] - r[1] * a[2][1]) - a[0][1] * (a[1][0] * r[2] - r[1] * a[2][0]) + r[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
  }
  if (det <= 0) return 0;
  for (int i = 0; i < n; i++) x[id[i]] = av1mi_fit_rdiv(128 * d[i], det);
  return 1;
}

// the taps first .. 2 of one pass (t[j] = 0 below `first`); returns 0 if absent.  *clamped: the taps the clamp acted on (bit j),
// *refit: the refit ran and gave a solution - what the tests count, null where nobody asks
AV1MI_FIT_HD inline int av1mi_wf_solve(const long long H[3][3], const long long R[3], int first, int t[3], int *clamped, int *refit) {
  const int all = first ? 6 : 7;
  long long x[3] = { 0, 0, 0 };
  t[0] = t[1] = t[2] = 0;
  if (clamped) *clamped = 0;
  if (refit) *refit = 0;
  if (!av1mi_wf_solve_idx(H, R, all, x)) return 0;
  int cl = 0;
  for (int j = first; j < 3; j++) {
    t[j] = av1mi_fit_clamp(x[j], av1mi_wiener_tap_min(j), av1mi_wiener_tap_max(j));
    if (t[j] != x[j]) cl |= 1 << j;
  }
  if (cl && cl != all) {
    long long R2[3] = { 0, 0, 0 }, y[3] = { 0, 0, 0 };
    for (int i = first; i < 3; i++) {
      long long acc = 0;
      for (int j = first; j < 3; j++) if ((cl >> j) & 1) acc += H[i][j] * t[j];
      R2[i] = R[i] - av1mi_fit_rdiv(acc, 128);
    }
    if (av1mi_wf_solve_idx(H, R2, all & ~cl, y)) {
      if (refit) *refit = 1;
      for (int j = first; j < 3; j++)
        if (!((cl >> j) & 1)) {
          t[j] = av1mi_fit_clamp(y[j], av1mi_wiener_tap_min(j), av1mi_wiener_tap_max(j));
          if (t[j] != y[j]) cl |= 8 << j;   // bits 3 .. 5: clamped by the refit
        }
    }
  }
  if (clamped) *clamped = cl;
  return 1;
}

// The unit's vertical (cv) and horizontal (ch) taps from its 27 sums; returns 0 if the candidate is absent.
// flags (or null): bits 0-5 the clamp bits of the vertical solve, 6-11 of the horizontal, 12 / 13 the refit ran in the vertical / horizontal
AV1MI_FIT_HD inline int av1mi_wiener_fit(const long long *sums, int first, int cv[3], int ch[3], int *flags) {
  long long Hvv[3][3], Hhh[3][3], Cv[3], R[3];
  for (int j = 0; j < 3; j++) {
    for (int k = 0; k < 3; k++) { Hvv[j][k] = sums[AV1MI_WF_HVV + av1mi_wf_sym(j, k)]; Hhh[j][k] = sums[AV1MI_WF_HHH + av1mi_wf_sym(j, k)]; }
    Cv[j] = sums[AV1MI_WF_CV + j];
  }
  int clv = 0, clh = 0, rfv = 0, rfh = 0;
  ch[0] = ch[1] = ch[2] = 0;
  if (flags) *flags = 0;
  if (!av1mi_wf_solve(Hvv, Cv, first, cv, &clv, &rfv)) return 0;
  for (int k = 0; k < 3; k++) {
    long long acc = 0;
    for (int j = 0; j < 3; j++) acc += sums[AV1MI_WF_HVH + j * 3 + k] * cv[j];
    R[k] = sums[AV1MI_WF_CH + k] - av1mi_fit_rdiv(acc, 128);
  }
  if (!av1mi_wf_solve(Hhh, R, first, ch, &clh, &rfh)) return 0;
  if (flags) *flags = clv | (clh << 6) | (rfv << 12) | (rfh << 13);
  return 1;
}

// A Wiener unit's bits (§5.11.58): pass 0 (the vertical filter) then pass 1 (the horizontal), taps first .. 2 of each as
// decode_signed_subexp_with_ref(Min_j, Max_j + 1, k = j + 1) against ref[pass][j] = RefLrWiener: at most 2 (6 + 7 + 8) = 42 bits.
// The caller carries the reference: after the unit it is the unit's taps.
AV1MI_FIT_HD inline Av1miBitString av1mi_lr_wiener_code(int first, const int cv[3], const int ch[3], const int ref[2][3]) {
  Av1miBitString b;
  for (int pass = 0; pass < 2; pass++)
    for (int j = first; j < 3; j++)
      lr_put_signed_ref(b, av1mi_wiener_tap_min(j), av1mi_wiener_tap_max(j) + 1, j + 1, ref[pass][j], pass ? ch[j] : cv[j]);
  return b;
}

#endif
