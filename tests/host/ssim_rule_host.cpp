// The quality pass's rule (av1-base_amd/csrc/ssim_rule.h: what quality_kernel.hip applies per window) compiled for the host, for
// tests/test_quality_host.py - as a shared object (the functions below) against the restatement tests/ssim_ref.py, and as a stand-alone
// program: reads cases from a text file, one per line, and prints one line of results each.
//   S bd s1 s2 ss s12            a window from its sums: A B Cn D w
//   W bd a[64] b[64]             a window from its samples, reference then test: s1 s2 ss s12 w
//   N n                          the windows along n samples
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../av1-base_amd/csrc/ssim_rule.h"

extern "C" int ssim_windows(int n) { return av1mi_ssim_windows(n); }
extern "C" unsigned ssim_c1(int bd) { return av1mi_ssim_c1(bd); }
extern "C" unsigned ssim_c2(int bd) { return av1mi_ssim_c2(bd); }
extern "C" int ssim_window(unsigned s1, unsigned s2, unsigned ss, unsigned s12, int bd) { return av1mi_ssim_window(s1, s2, ss, s12, bd); }
extern "C" void ssim_factors(unsigned s1, unsigned s2, unsigned ss, unsigned s12, int bd, long long out[4]) {
  const Av1miSsimFactors F = av1mi_ssim_factors(s1, s2, ss, s12, bd);
  out[0] = (long long)F.A; out[1] = (long long)F.B; out[2] = (long long)F.Cn; out[3] = (long long)F.D;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char t;
  long lines = 0;
  while (fscanf(f, " %c", &t) == 1) {
    const int want = t == 'S' ? 5 : t == 'W' ? 129 : t == 'N' ? 1 : -1;
    if (want < 0) { fprintf(stderr, "line %ld: unknown case '%c'\n", lines, t); fclose(f); return 2; }
    std::vector<long long> a((size_t)want);
    for (int i = 0; i < want; i++)
      if (fscanf(f, "%lld", &a[(size_t)i]) != 1) { fprintf(stderr, "short line %ld\n", lines); fclose(f); return 2; }
    if (t == 'S') {
      const uint32_t s1 = (uint32_t)a[1], s2 = (uint32_t)a[2], ss = (uint32_t)a[3], s12 = (uint32_t)a[4];
      const Av1miSsimFactors F = av1mi_ssim_factors(s1, s2, ss, s12, (int)a[0]);
      printf("%" PRIu64 " %" PRIu64 " %" PRId64 " %" PRIu64 " %d\n", F.A, F.B, F.Cn, F.D, (int)av1mi_ssim_window(s1, s2, ss, s12, (int)a[0]));
    } else if (t == 'W') {
      uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
      for (size_t k = 0; k < 64; k++) {
        const uint32_t x = (uint32_t)a[1 + k], y = (uint32_t)a[65 + k];
        s1 += x; s2 += y; ss += x * x + y * y; s12 += x * y;
      }
      printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d\n", s1, s2, ss, s12, (int)av1mi_ssim_window(s1, s2, ss, s12, (int)a[0]));
    } else {
      printf("%d\n", av1mi_ssim_windows((int)a[0]));
    }
    lines++;
  }
  fclose(f);
  return 0;
}
