// Host-side check of the compact CDF image (av1mi_dev.h: Av1miCdfCompact, av1mi_cdf_compact_build), built as plain C++ by
// tests/test_cdf_compact_host.py: for leaves of 8 .. 64 samples the image the host uploads behind the blob equals what every wave of
// the regular symbolize variants used to gather from the blob for itself - that gather is restated here, lane by lane, as the kernel
// had it - in both plane types' slices, and its tail is zero.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../av1-base_amd/csrc/av1mi_dev.h"

typedef Av1miCdfLayout CL;
typedef Av1miCdfCompact CC;

// the kernel's former prologue: 64 lanes, each statement over `lane`
static void gather(const uint16_t *cdf_init, int max_bs_log2, uint16_t *w) {
  const int l2y = max_bs_log2 > 6 ? 6 : max_bs_log2, l2c = l2y - 1 > 5 ? 5 : l2y - 1;
  for (int lane = 0; lane < 64; lane++) {
    for (int i = lane; i < CC::LEAD; i += 64) w[i] = cdf_init[i];
    for (int i = lane; i < 13 * 8; i += 64)
      w[CC::TXSET + i] = l2y <= 3 ? cdf_init[CL::TX_SET1 + (l2y - 2) * 13 * 8 + i] : ((l2y == 4 && i < 13 * 6) ? cdf_init[CL::TX_SET2 + (l2y - 2) * 13 * 6 + i] : (uint16_t)0);
    for (int i = lane; i < 2 * 39; i += 64) { const int p = i / 39, txs = (p ? l2c : l2y) - 2; w[CC::TXB_SKIP + i] = cdf_init[CL::TXB_SKIP + txs * 39 + i % 39]; }
    if (lane < 24) {
      const int p = lane / 12, k = lane % 12, bwl = (p ? l2c : l2y) > 5 ? 5 : (p ? l2c : l2y), msz = 2 * bwl - 4, nsy = 5 + msz;
      const int eoff = CL::EOB16 + 4 * (msz * 6 + (msz * (msz - 1)) / 2) + (p * 2 + 0) * (nsy + 1);
      w[CC::EOB + lane] = k <= nsy ? cdf_init[eoff + k] : (uint16_t)0;
    }
    if (lane < 2 * 27) { const int p = lane / 27, txs = (p ? l2c : l2y) - 2; w[CC::EOB_EXTRA + lane] = cdf_init[CL::EOB_EXTRA + (txs * 2 + p) * 27 + lane % 27]; }
    if (lane < 18) w[CC::DC_SIGN + lane] = cdf_init[CL::DC_SIGN + lane];
    if (lane < 2 * 16) { const int p = lane / 16, txs = (p ? l2c : l2y) - 2; w[CC::COEFF_BASE_EOB + lane] = cdf_init[CL::COEFF_BASE_EOB + (txs * 2 + p) * 16 + lane % 16]; }
    for (int i = lane; i < CC::TOTAL - CC::USE_WIENER; i += 64) w[CC::USE_WIENER + i] = cdf_init[CL::USE_WIENER + i];
    if (lane < 18) w[CC::TOTAL + lane] = 0;
  }
}

int main() {
  // a blob in which every entry differs from its neighbours and from the same entry of another table: a wrong slice shows
  std::vector<uint16_t> blob(CC::BLOB_WORDS, 0);
  for (int i = 0; i < CL::TOTAL; i++) blob[i] = (uint16_t)(1 + (i * 40503u) % 65521u);
  static_assert(CC::AT % 8 == 0 && CC::WORDS % 8 == 0 && CC::AT >= CL::TOTAL && CC::WORDS >= CC::TOTAL + 18, "whole 16-byte pieces behind the blob");
  int checked = 0;
  for (int l2 = 3; l2 <= 6; l2++) {
    std::vector<uint16_t> want(CC::WORDS, 0xABCD), got(CC::WORDS, 0x1234);
    gather(blob.data(), l2, want.data());
    for (int i = CC::TOTAL + 18; i < CC::WORDS; i++) want[i] = 0;   // (the padding up to a whole piece)
    av1mi_cdf_compact_build(blob.data(), l2, got.data());
    for (int i = 0; i < CC::WORDS; i++)
      if (want[i] != got[i]) { printf("leaf 2^%d: entry %d is %u, the gather gives %u\n", l2, i, got[i], want[i]); return 1; }
    // both plane types' slices are there and are not the same slice (except where the sizes share a table)
    const int l2c = l2 - 1 > 5 ? 5 : l2 - 1;
    for (int p = 0; p < 2; p++) {
      const int txs = (p ? l2c : l2) - 2;
      if (got[CC::TXB_SKIP + p * 39] != blob[CL::TXB_SKIP + txs * 39] || got[CC::EOB_EXTRA + p * 27 + 26] != blob[CL::EOB_EXTRA + (txs * 2 + p) * 27 + 26] ||
          got[CC::COEFF_BASE_EOB + p * 16 + 15] != blob[CL::COEFF_BASE_EOB + (txs * 2 + p) * 16 + 15]) { printf("leaf 2^%d plane type %d: wrong slice\n", l2, p); return 1; }
    }
    // the image in place behind the blob, as the host uploads it
    av1mi_cdf_compact_build(blob.data(), l2, blob.data() + CC::AT);
    for (int i = 0; i < CC::WORDS; i++) if (blob[CC::AT + i] != want[i]) { printf("leaf 2^%d: in place, entry %d\n", l2, i); return 1; }
    checked++;
  }
  printf("ok %d\n", checked);
  return 0;
}
