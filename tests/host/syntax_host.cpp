// The host code that needs no GPU (av1-base_amd/csrc/av1mi_syntax.cpp) as a stand-alone program for the plain host compiler, with and
// without sanitizers (tests/test_syntax_host.py): reads parameter sets - the 36 words of av1mi_params per line - and prints for each
// what resolve() makes of it, the headers, and checksums of the default CDF blob and of the kernels' parameters.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../av1-base_amd/csrc/av1mi_syntax.h"

using namespace av1mi;

static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
  return h;
}
static void hex(const char *tag, const std::vector<uint8_t> &v) {
  printf(" %s=", tag);
  for (uint8_t b : v) printf("%02x", b);
}

int main(int argc, char **argv) {
  static_assert(sizeof(av1mi_params) == 36 * sizeof(uint32_t), "av1mi_params is 36 words");
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: syntax_host <file of parameter sets>\n"); return 2; }
  for (;;) {
    uint32_t w[36];
    int n = 0;
    while (n < 36 && fscanf(f, "%u", &w[n]) == 1) n++;
    if (n == 0) break;
    if (n != 36) { fprintf(stderr, "short parameter set\n"); return 2; }
    av1mi_params p;
    memcpy(&p, w, sizeof(p));
    Resolved r;
    memset(&r, 0, sizeof(r));
    const int rc = resolve(&p, &r);
    printf("rc=%d", rc);
    if (rc) { printf("\n"); continue; }
    printf(" cq=%u aq=%d tf_frames=%d tf_strength=%d presearch=%u lr=%u lr_chroma=%d lr_unit_shift=%d lr_rd=%d lr_fit_mask=%u lr_wfit=%d", r.p.cq_level, r.aq,
           r.tf_frames, r.tf_strength, r.p.me_presearch, r.p.enable_lr, r.lr_chroma, r.lr_unit_shift, r.lr_lambda ? 1 : 0, r.lr_fit_mask, r.lr_wfit);
    printf(" qidx=%d cw=%d ch=%d padded=%d sb=%dx%d tile_sb=%d tiles=%dx%d qm_level=%d keyint=%u me_range=%u block_log2=%u min_block_log2=%u damping=%u", r.qidx, r.cw,
           r.ch, r.padded ? 1 : 0, r.sb_cols, r.sb_rows, r.tile_sb, r.tile_cols, r.tile_rows, r.qm_level, r.p.keyint, r.p.me_range, r.p.block_log2, r.p.min_block_log2,
           r.p.cdef_damping);
    hex("seq", make_sequence_header(r));
    for (int inter = 0; inter < 2; inter++) {
      size_t bits = 0, cdef_bit = 0, lf_bit = 0;
      const std::vector<uint8_t> h = make_frame_header(r, &bits, 0, inter != 0, &cdef_bit, &lf_bit);
      printf(" %s_bits=%zu %s_cdef_bit=%zu %s_lf_bit=%zu", inter ? "inter" : "key", bits, inter ? "inter" : "key", cdef_bit, inter ? "inter" : "key", lf_bit);
      hex(inter ? "inter" : "key", h);
    }
    const std::vector<uint16_t> cdf = make_cdf_blob(r.qidx);
    printf(" cdf_words=%zu cdf_sum=%016llx", cdf.size(), (unsigned long long)fnv(cdf.data(), cdf.size() * 2));
    const Av1miDevParams P = dev_params(r, 3, 1);
    printf(" dev_sum=%016llx stream_cap=%d\n", (unsigned long long)fnv(&P, sizeof(P)), tile_stream_cap(r, 1));
  }
  fclose(f);
  return 0;
}
