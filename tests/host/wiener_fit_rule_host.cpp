// The Wiener fit's rule header (av1-base_amd/csrc/wiener_fit_rule.h) compiled for the host: tests/test_wiener_fit_host.py checks the
// solve and the unit-code writer against the Python restatement (tests/wiener_fit_ref.py).  With -DWIENER_FIT_RULE_MAIN a stand-alone
// program that runs the rule over generated sums up to the 2^36 bound - what the sanitizer build executes.
#include "../../av1-base_amd/csrc/wiener_fit_rule.h"

// n problems: sums[27 n], first[n] -> taps[6 n] (cv, ch), present[n], flags[n]
extern "C" void wf_fit(const long long *sums, const int *first, int n, int *taps, int *present, int *flags) {
  for (int i = 0; i < n; i++) present[i] = av1mi_wiener_fit(sums + AV1MI_LR_WFIT_SUMS * i, first[i], taps + 6 * i, taps + 6 * i + 3, flags + i);
}
// one pass: H[9] (row major), R[3] -> t[3]; returns present
extern "C" int wf_solve(const long long *H, const long long *R, int first, int *t, int *clamped, int *refit) {
  long long h[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) h[i][j] = H[i * 3 + j];
  return av1mi_wf_solve(h, R, first, t, clamped, refit);
}
extern "C" int wf_code(int first, const int *cv, const int *ch, const int *ref, unsigned long long *bits) {
  int r[2][3];
  for (int p = 0; p < 2; p++) for (int j = 0; j < 3; j++) r[p][j] = ref[p * 3 + j];
  const Av1miBitString b = av1mi_lr_wiener_code(first, cv, ch, r);
  *bits = b.bits;
  return b.len;
}
// every (reference, value) pair of tap j as a one-tap code: bits[n * n], len likewise, n = Max_j - Min_j + 1
extern "C" void wf_tap_table(int j, unsigned long long *bits, int *len) {
  const int lo = av1mi_wiener_tap_min(j), n = av1mi_wiener_tap_max(j) - lo + 1;
  for (int r = 0; r < n; r++)
    for (int v = 0; v < n; v++) {
      Av1miBitString b;
      lr_put_signed_ref(b, lo, lo + n, j + 1, lo + r, lo + v);
      bits[r * n + v] = b.bits; len[r * n + v] = b.len;
    }
}

#ifdef WIENER_FIT_RULE_MAIN
#include <stdio.h>
#include <initializer_list>
int main() {
  unsigned long long seed = 88172645463325252ull;
  auto next = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  long failures = 0, present = 0, longest = 0;
  const int cases = 200000;
  for (int it = 0; it < cases; it++) {
    long long sums[AV1MI_LR_WFIT_SUMS];
    const int bits = 1 + (int)(next() % 36);
    const long long mag = (1ll << bits) - (it % 7 == 0 ? 0 : 1);   // every seventh case at the bound itself
    for (int k = 0; k < AV1MI_LR_WFIT_SUMS; k++) {
      const long long v = (long long)(next() % (unsigned long long)(mag + 1));
      sums[k] = (it % 5 == 0) ? (next() & 1 ? mag : -mag) : (next() & 1 ? v : -v);
    }
    if (it % 3) for (int k : { 0, 3, 5, 6, 9, 11 }) sums[k] = sums[k] < 0 ? -sums[k] : sums[k];   // diagonals as sums of squares
    int cv[3], ch[3], flags;
    const int first = it & 1;
    if (!av1mi_wiener_fit(sums, first, cv, ch, &flags)) continue;
    present++;
    for (int j = 0; j < 3; j++)
      for (const int *t : { cv, ch })
        if (t[j] < (j < first ? 0 : av1mi_wiener_tap_min(j)) || t[j] > (j < first ? 0 : av1mi_wiener_tap_max(j))) failures++;
    int ref[2][3];
    for (int p = 0; p < 2; p++) for (int j = 0; j < 3; j++) ref[p][j] = av1mi_wiener_tap_min(j) + (int)(next() % (unsigned)(av1mi_wiener_tap_max(j) - av1mi_wiener_tap_min(j) + 1));
    const Av1miBitString b = av1mi_lr_wiener_code(first, cv, ch, ref);
    if (b.len > 64 || b.len <= 0) failures++;
    longest = b.len > longest ? b.len : longest;
  }
  printf("%d cases, %ld present, longest code %ld bits, %ld failures\n", cases, present, longest, failures);
  return failures != 0;
}
#endif
