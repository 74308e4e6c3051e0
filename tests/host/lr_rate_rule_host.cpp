// The restoration decisions' rate rule (av1-base_amd/csrc/lr_rate_rule.h) compiled for the host, a stand-alone program:
// tests/test_lr_rd_host.py compares what it prints with the Python restatement (tests/lr_rd_ref.py) and runs it a second time under
// the sanitizers.  It prints
//   CDF ok                           the header's probabilities are av1_tables.h's default CDFs (else the program fails)
//   T16 a b c d e                    NONE, WIENER, SGRPROJ on a switchable plane, off, on on a Wiener-only one
//   WY c0 c1 : 64 lengths            Lc of the luma filter with taps (c0, c1, c2) in both passes, c2 over its range
//   WC c1 : 64 lengths               the same for chroma (tap 0 is 0 and not coded)
//   S set x0 : lengths               Lc of the self-guided unit (set, x0, x1), x1 over the grid
//   LAM bd s : 255 values            lambda of base_q_idx 1 .. 255
#include <stdio.h>
#include "../../av1-base_amd/csrc/av1_tables.h"
#include "../../av1-base_amd/csrc/lr_rate_rule.h"

static_assert(av1mi_lr_type_t16(1, 0) == 30 && av1mi_lr_type_t16(1, 1) == 23 && av1mi_lr_type_t16(1, 2) == 29, "switchable planes");
static_assert(av1mi_lr_type_t16(0, 0) == 26 && av1mi_lr_type_t16(0, 1) == 12, "Wiener-only planes");

// the weights' grid: every seventh value and both clamps
static int grid(int lo, int hi, int *out) {
  int n = 0;
  for (int v = lo; v < hi; v += 7) out[n++] = v;
  out[n++] = hi;
  return n;
}

int main() {
  if (av1_default_switchable_restore_cdf[0][0] != AV1MI_LR_CDF_SWITCHABLE_0 || av1_default_switchable_restore_cdf[0][1] != AV1MI_LR_CDF_SWITCHABLE_1 ||
      av1_default_use_wiener_cdf[0][0] != AV1MI_LR_CDF_USE_WIENER) {
    printf("CDF mismatch\n");
    return 1;
  }
  printf("CDF ok\n");
  printf("T16 %d %d %d %d %d\n", av1mi_lr_type_t16(1, 0), av1mi_lr_type_t16(1, 1), av1mi_lr_type_t16(1, 2), av1mi_lr_type_t16(0, 0), av1mi_lr_type_t16(0, 1));
  for (int first = 0; first < 2; first++)
    for (int c0 = first ? 0 : av1mi_wiener_tap_min(0); c0 <= (first ? 0 : av1mi_wiener_tap_max(0)); c0++)
      for (int c1 = av1mi_wiener_tap_min(1); c1 <= av1mi_wiener_tap_max(1); c1++) {
        if (first) printf("WC %d :", c1); else printf("WY %d %d :", c0, c1);
        for (int c2 = av1mi_wiener_tap_min(2); c2 <= av1mi_wiener_tap_max(2); c2++) {
          const int c[3] = { c0, c1, c2 }, mid[2][3] = { { 3, -7, 15 }, { 3, -7, 15 } };
          const int lc = av1mi_lr_wiener_lc(first, c0, c1, c2, c0, c1, c2);
          if (lc != av1mi_lr_wiener_code(first, c, c, mid).len) return 2;   // the count is the writer's length
          printf(" %d", lc);
        }
        printf("\n");
      }
  int g0[32], g1[32];
  const int n0 = grid(AV1MI_SGR_XQD0_MIN, AV1MI_SGR_XQD0_MAX, g0), n1 = grid(AV1MI_SGR_XQD1_MIN, AV1MI_SGR_XQD1_MAX, g1);
  for (int t = 0; t < AV1MI_LR_FIT_SETS; t++)
    for (int i = 0; i < n0; i++) {
      printf("S %d %d :", t, g0[i]);
      for (int j = 0; j < n1; j++) {
        if (av1mi_lr_sgr_lc(t, g0[i], g1[j]) != av1mi_lr_sgr_code(t, g0[i], g1[j], -32, 31).len) return 2;
        printf(" %d", av1mi_lr_sgr_lc(t, g0[i], g1[j]));
      }
      printf("\n");
    }
  for (int bd = 8; bd <= 10; bd += 2)
    for (int s = 0; s < 4; s++) {
      printf("LAM %d %d :", bd, s);
      for (int q = 1; q < 256; q++) printf(" %llu", av1mi_lr_lambda_of_step((unsigned long long)(bd == 8 ? av1_dc_q8[q] : av1_dc_q10[q]), s));
      printf("\n");
    }
  // the bounds of J: the largest lambda times the largest B16 stays below 2^32
  const unsigned long long top = av1mi_lr_lambda_of_step((unsigned long long)av1_dc_q10[255], 3) * (unsigned long long)av1mi_lr_b16(42, 30);
  printf("BOUND %llu\n", top);
  return top < (1ull << 32) ? 0 : 1;
}
