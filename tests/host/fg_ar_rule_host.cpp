// The film grain's autoregressive fit (av1-base_amd/csrc/fg_ar_rule.h) compiled for the host, as a stand-alone program:
// tests/test_fg_ar_host.py writes the cases, runs it - plain and under the sanitizers - and checks the lines against the restatement
// (tests/fg_ar_ref.py).  Linked with av1-base_amd/csrc/av1mi_syntax.cpp for the frame headers of both kinds.
//   B bd n lag q x[n * n]         a block of n x n samples and its bin's quartile  ->  sum e^2, the energy condition, the block's 46 sums
//   C rec pl quart[8] count[8]    a block record, a plane, its quartiles and counts ->  whether the block is a candidate
//   F lag n flat R[46]            a plane's sums and flat blocks                    ->  present, the 25 coefficients, the gain
//   H p[36] frame inter           av1mi_params as 36 words, a frame number, the kind ->  rc, the header's bits, fg_bit, fg_ar_bit, the header in hex
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../av1-base_amd/csrc/av1mi_syntax.h"
#include "../../av1-base_amd/csrc/fg_ar_rule.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'B') {
      int bd, n, lag, q;
      if (fscanf(f, "%d %d %d %d", &bd, &n, &lag, &q) != 4 || (n != 8 && n != 16) || lag < 1 || lag > AV1MI_FGAR_MAX_LAG) return 3;
      std::vector<uint16_t> x((size_t)n * n);
      for (auto &v : x) { unsigned u; if (fscanf(f, "%u", &u) != 1) return 3; v = (uint16_t)u; }
      std::vector<int> e((size_t)n * n);
      const uint64_t en = av1mi_fgar_block_noise(x.data(), (size_t)n, n, e.data());
      long long R[AV1MI_FGAR_SUMS] = {};
      av1mi_fgar_block_sums(e.data(), n, lag, R);
      printf("%llu %d", (unsigned long long)en, av1mi_fgar_energy_ok(en, n, q, bd) ? 1 : 0);
      for (long long v : R) printf(" %lld", v);
      printf("\n");
    } else if (kind == 'C') {
      unsigned rec;
      int pl, quart[8];
      uint32_t count[8];
      if (fscanf(f, "%x %d", &rec, &pl) != 2 || pl < 0 || pl > 2) return 3;
      for (int &v : quart) if (fscanf(f, "%d", &v) != 1) return 3;
      for (uint32_t &v : count) if (fscanf(f, "%u", &v) != 1) return 3;
      printf("%d\n", av1mi_fgar_candidate(rec, pl, quart, count) ? 1 : 0);
    } else if (kind == 'F') {
      int lag, n;
      unsigned flat;
      long long R[AV1MI_FGAR_SUMS];
      if (fscanf(f, "%d %d %u", &lag, &n, &flat) != 3 || (n != 8 && n != 16) || lag < 1 || lag > AV1MI_FGAR_MAX_LAG) return 3;
      for (long long &v : R) if (fscanf(f, "%lld", &v) != 1) return 3;
      int rho[AV1MI_FGAR_SUMS];
      std::vector<long long> ws(AV1MI_FGAR_WS, 0);
      int8_t c[AV1MI_FGAR_COEFFS];
      uint32_t gain = 0;
      printf("%d", av1mi_fgar_fit(lag, R, flat, n, rho, false, ws.data(), c, &gain));
      for (int8_t v : c) printf(" %d", (int)v);
      printf(" %u\n", gain);
    } else if (kind == 'H') {
      uint32_t w[36];
      unsigned frame, inter;
      for (auto &v : w) if (fscanf(f, "%u", &v) != 1) return 3;
      if (fscanf(f, "%u %u", &frame, &inter) != 2) return 3;
      av1mi_params p;
      static_assert(sizeof(p) == sizeof(w), "av1mi_params is 36 words");
      memcpy(&p, w, sizeof(p));
      av1mi::Resolved r;
      memset(&r, 0, sizeof(r));
      const int rc = av1mi::resolve(&p, &r);
      if (rc) { printf("%d\n", rc); continue; }
      size_t bits = 0, fg_bit = 0, ar_bit = 0;
      const std::vector<uint8_t> h = av1mi::make_frame_header(r, &bits, frame, inter != 0, nullptr, nullptr, &fg_bit, &ar_bit);
      printf("0 %zu %zu %zu ", bits, fg_bit, ar_bit);
      for (uint8_t b : h) printf("%02x", b);
      printf("\n");
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
