// The self-guided fit's rule header (av1-base_amd/csrc/lr_fit_rule.h) compiled for the host: tests/test_lr_fit_host.py checks the
// parameter table, the solve and the unit-code writer against the Python restatement (tests/sgr_fit_ref.py).
#include "../../av1-base_amd/csrc/lr_fit_rule.h"

extern "C" void fit_params(int t, int *out) { out[0] = av1mi_sgr_r0(t); out[1] = av1mi_sgr_eps0(t); out[2] = av1mi_sgr_r1(t); out[3] = av1mi_sgr_eps1(t); }
// n problems: sums[5 n] -> w[2 n], present[n]
extern "C" void fit_solve(const int *t, const long long *sums, int n, int *w, int *present) {
  for (int i = 0; i < n; i++) present[i] = av1mi_lr_fit_solve(t[i], sums + 5 * i, &w[2 * i], &w[2 * i + 1]);
}
extern "C" int fit_code(int set, int xqd0, int xqd1, int ref0, int ref1, unsigned long long *bits) {
  const Av1miBitString b = av1mi_lr_sgr_code(set, xqd0, xqd1, ref0, ref1);
  *bits = b.bits;
  return b.len;
}
// every (reference, value) pair of weight i of set `set` (the other weight and its reference held at `other`): bits[128 * 128], len likewise
extern "C" void fit_code_table(int set, int i, int other, unsigned long long *bits, int *len) {
  const int lo = i ? AV1MI_SGR_XQD1_MIN : AV1MI_SGR_XQD0_MIN;
  for (int r = 0; r < 128; r++)
    for (int v = 0; v < 128; v++) {
      const Av1miBitString b = i ? av1mi_lr_sgr_code(set, other, lo + v, other, lo + r) : av1mi_lr_sgr_code(set, lo + v, other, lo + r, other);
      bits[r * 128 + v] = b.bits; len[r * 128 + v] = b.len;
    }
}
