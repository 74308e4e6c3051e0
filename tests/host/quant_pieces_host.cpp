// Host build of the reconstruction kernel's quantiser rule (av1-base_amd/csrc/quant_pieces.h) for tests/test_quant_pieces_host.py: the same
// source the kernel compiles, against the oracle's quantiser - the loop over a block's coefficients in oracle/av1o_enc.c
// (code_tx_block), restated here per coefficient in 64-bit arithmetic because the oracle has it inside the block coder.  Test
// infrastructure only.  The restatement is tied to the oracle itself by tests/test_recon_trim.py, which compares what the kernel codes
// with this header against the oracle's bitstream and reconstruction.  With -DQUANT_PIECES_MAIN the file is a program of its own that runs every check and prints the mismatches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../av1-base_amd/csrc/quant_pieces.h"
#include "../../av1-base_amd/csrc/av1_tables.h"

namespace qp = av1mi_quant;

// ---- the oracle's rule (oracle/av1o_enc.c, code_tx_block: "dead-zone quantise" and "normative dequant §7.12.3")
static int ref_tsh(int log2n) { return log2n >= 6 ? 2 : (log2n == 5 ? 1 : 0); }
static uint32_t ref_rnd(uint32_t q, int i, int j, int cw) { return (i + j) < (cw >> 2) ? (3 * q) >> 3 : ((i + j) < (cw >> 1) ? (q >> 2) : (q >> 3)); }
static int32_t ref_level(int32_t v, uint32_t q, uint32_t rnd, int sh) {
  const uint32_t recip = (uint32_t)((((uint64_t)1 << 32) + q - 1) / q);
  const uint32_t a = ((uint32_t)llabs((long long)v) << sh) + rnd;
  uint32_t lv = (uint32_t)(((uint64_t)a * recip) >> 32);
  if (lv > 0x7FFF) lv = 0x7FFF;
  return v < 0 ? -(int32_t)lv : (int32_t)lv;
}
static int32_t ref_dequant(int32_t lv, uint32_t q, int sh, int bd) {
  int64_t d = ((int64_t)llabs((long long)lv) * q) & 0xFFFFFF;
  const int64_t lim = (int64_t)1 << (7 + bd);
  d >>= sh;
  if (lv < 0) d = -d;
  if (d < -lim) d = -lim;
  if (d > lim - 1) d = lim - 1;
  return (int32_t)d;
}

template <int TSH>
static long sweep_t(int bd, uint32_t q, int cls, long *capped) {
  const uint32_t recip = (uint32_t)((((uint64_t)1 << 32) + q - 1) / q);
  const int lim = 1 << (7 + bd);
  // a position of the class in a 32-wide area, for the reference's own class rule
  const int i = cls == 0 ? 0 : (cls == 1 ? 8 : 16), j = 0;
  const uint32_t rnd = qp::dz_round(q, cls);
  long bad = rnd != ref_rnd(q, i, j, 32);
  static const int32_t extremes[] = { 1 << 17, (1 << 17) + 1, 1 << 18, (1 << 19) - 1, 1 << 20, (1 << 22) + 12345, 1 << 23, (1 << 24) - 1, 1 << 26, 1 << 28, (1 << 29) - 1 };
  const int NE = (int)(sizeof(extremes) / sizeof(extremes[0]));
  for (long k = -65536 - 2 * NE; k <= 65536; k++) {
    int32_t v = (int32_t)k;
    if (k < -65536) { const long e = -65537 - k; v = (e & 1) ? -extremes[e >> 1] : extremes[e >> 1]; }
    // the unified step - what every quantiser loop of the kernel calls - and its two halves on their own: the level alone (the matrix-core
    // loop) and the stored level through the dequantiser (the row pass that follows it)
    const qp::Quantised z = qp::quantise_dequantise<TSH>(v, q, recip, rnd, lim), z0 = qp::quantise<TSH>(v, rnd, recip);
    const int32_t want = ref_level(v, q, rnd, TSH), want_d = ref_dequant(want, q, TSH, bd);
    bad += z.level != want || (int16_t)z.level != want || z.mag != (uint32_t)llabs((long long)want);
    bad += z.deq != want_d;
    bad += z0.level != want || z0.mag != z.mag || z0.deq != 0;
    bad += qp::dequant_level<TSH>((int16_t)z.level, q, lim) != want_d;
    *capped += z.mag == qp::LEVEL_CAP;
  }
  return bad;
}

static long sweep(int log2n, int bd, uint32_t q, int cls, long *capped) {
  const int sh = ref_tsh(log2n);
  return sh == 0 ? sweep_t<0>(bd, q, cls, capped) : (sh == 1 ? sweep_t<1>(bd, q, cls, capped) : sweep_t<2>(bd, q, cls, capped));
}

// every coefficient value in +-2^16 and the extremes, both steps of the quantiser index, the three dead-zone classes: mismatches
extern "C" long qp_sweep(int log2n, int bd, int qidx, long *capped) {
  const uint32_t qs[2] = { (uint32_t)(bd == 8 ? av1_dc_q8[qidx] : av1_dc_q10[qidx]), (uint32_t)(bd == 8 ? av1_ac_q8[qidx] : av1_ac_q10[qidx]) };
  long bad = 0;
  *capped = 0;
  for (int s = 0; s < 2; s++)
    for (int cls = 0; cls < 3; cls++) bad += sweep(log2n, bd, qs[s], cls, capped);
  return bad;
}

// ---- quantiser-matrix steps: Round2(q * Quantizer_Matrix, 5) as the context's table holds them (av1mi_syntax.cpp, make_qm_table)
static uint32_t qm_step(uint32_t q, uint32_t entry) { return (q * entry + 16) >> 5; }
static void qm_entry_range(uint32_t *lo, uint32_t *hi) {
  *lo = 255; *hi = 0;
  for (int l = 0; l < 15; l++)
    for (int pt = 0; pt < 2; pt++)
      for (int i = 0; i < 1360; i++) {
        const uint32_t e = av1_qm_iwt[l][pt][i];
        *lo = e < *lo ? e : *lo; *hi = e > *hi ? e : *hi;
      }
}
// the largest step a table can hold at the bit depth (any matrix level, plane type and position, the highest quantiser index), and the
// range of the matrix entries: what q_mul24's "both operands below 2^24" rests on
extern "C" uint32_t qp_qm_max_step(int bd, uint32_t *entry_lo, uint32_t *entry_hi) {
  qm_entry_range(entry_lo, entry_hi);
  uint32_t top = 0;
  for (int qidx = 0; qidx < 256; qidx++)
    for (int l = 0; l < 15; l++)
      for (int pt = 0; pt < 2; pt++)
        for (int i = 0; i < 1360; i++) {
          const bool dc = i == 0 || i == 16 || i == 80 || i == 336;   // the first position of each size
          const uint32_t q = (uint32_t)(bd == 8 ? (dc ? av1_dc_q8 : av1_ac_q8)[qidx] : (dc ? av1_dc_q10 : av1_ac_q10)[qidx]);
          const uint32_t st = qm_step(q, av1_qm_iwt[l][pt][i]);
          top = st > top ? st : top;
        }
  return top;
}
// the sweep of qp_sweep at the extreme steps of the quantiser-matrix tables: smallest and largest matrix entry on both steps of the index
extern "C" long qp_sweep_qm(int log2n, int bd, int qidx, long *capped) {
  const uint32_t qs[2] = { (uint32_t)(bd == 8 ? av1_dc_q8[qidx] : av1_dc_q10[qidx]), (uint32_t)(bd == 8 ? av1_ac_q8[qidx] : av1_ac_q10[qidx]) };
  uint32_t e[2];
  qm_entry_range(&e[0], &e[1]);
  long bad = 0;
  *capped = 0;
  for (int s = 0; s < 2; s++)
    for (int k = 0; k < 2; k++)
      for (int cls = 0; cls < 3; cls++) bad += sweep(log2n, bd, qm_step(qs[s], e[k]), cls, capped);
  return bad;
}

template <int CW>
static long rows_t() {
  const uint32_t q = 1000, r0 = qp::dz_round(q, 0), r1 = qp::dz_round(q, 1), r2 = qp::dz_round(q, 2);
  long bad = 0;
  for (int row = 0; row < CW; row++) {
    const int ta = qp::dz_ta(row, CW), tb = qp::dz_tb(row, CW);
    for (int j = 0; j < CW; j++) {
      const uint32_t want = ref_rnd(q, row, j, CW);
      bad += qp::dz_round(q, qp::dz_class(row, j, CW)) != want;
      bad += qp::dz_pick(j, ta, tb, r0, r1, r2) != want;
      bad += qp::dz_round_row<CW>(j, ta, tb, r0, r1, r2) != want;
    }
  }
  return bad;
}

// every (row, column): the class and its per-lane forms (a row per lane at every coded width; the matrix-core layout at 32x32), the key
// and the extent of a lane from its last nonzero position
extern "C" long qp_positions(void) {
  long bad = rows_t<4>() + rows_t<8>() + rows_t<16>() + rows_t<32>();
  const uint32_t q = 1000, r0 = qp::dz_round(q, 0), r1 = qp::dz_round(q, 1), r2 = qp::dz_round(q, 2);
  bool seen[32][32] = {};
  for (int lane = 0; lane < 64; lane++) {
    const int col = lane & 31, mh = lane >> 5;
    const int ta = qp::dz_ta(col + 4 * mh, 32), tb = qp::dz_tb(col + 4 * mh, 32);
    int prev_row = -1, prev_key = -1;
    for (int reg = 0; reg < 16; reg++) {
      const int row = qp::mm_row(reg, mh);
      bad += row <= prev_row || row > 31 || seen[row][col];   // rows grow with the register; every position once
      seen[row][col] = true;
      bad += qp::dz_round_mm(reg, ta, tb, r0, r1, r2) != ref_rnd(q, row, col, 32);
      bad += qp::scan_key(row, col) <= prev_key;              // ... and so does the key: the last nonzero register decides it
      prev_row = row; prev_key = qp::scan_key(row, col);
    }
  }
  for (int r = 0; r < 32; r++)
    for (int c = 0; c < 32; c++) {
      bad += !seen[r][c];
      bad += qp::extent(r, c) != (((uint32_t)(r + 1) << 16) | (uint32_t)(c + 1));
      if (c) bad += qp::scan_key(r, c) <= qp::scan_key(r, c - 1);   // a row per lane: the key grows with the column
      if (r) bad += qp::scan_key(r, c) <= qp::scan_key(r - 1, c);
    }
  return bad;
}

// scan keys of a cw x cw area, row-major
extern "C" void qp_keys(int cw, int *out) {
  for (int r = 0; r < cw; r++)
    for (int c = 0; c < cw; c++) out[r * cw + c] = qp::scan_key(r, c);
}

// scan indices of a cw x cw block, row-major; the formula is a constant expression too (the symbolizer builds its table from it)
static_assert(qp::scan_index(0, 0, 4) == 0 && qp::scan_index(0, 1, 4) == 1 && qp::scan_index(1, 0, 4) == 2 && qp::scan_index(3, 3, 4) == 15, "zig-zag");
extern "C" void qp_scan_indices(int cw, int *out) {
  for (int r = 0; r < cw; r++)
    for (int c = 0; c < cw; c++) out[r * cw + c] = qp::scan_index(r, c, cw);
}

#ifdef QUANT_PIECES_MAIN
int main() {
  long bad = qp_positions(), capped_all = 0;
  static const int qidx[] = { 1, 120, 255 };
  for (int log2n = 2; log2n <= 6; log2n++)
    for (int bd = 8; bd <= 10; bd += 2)
      for (int k = 0; k < 3; k++) {
        long capped = 0;
        bad += qp_sweep(log2n, bd, qidx[k], &capped);
        capped_all += capped;
        if (log2n <= 5) { bad += qp_sweep_qm(log2n, bd, qidx[k], &capped); capped_all += capped; }   // (the matrices stop at 32x32)
      }
  if (!capped_all) bad++;
  uint32_t lo, hi;
  bad += qp_qm_max_step(8, &lo, &hi) >= (1u << 16) || qp_qm_max_step(10, &lo, &hi) >= (1u << 16);
  printf("quant_pieces: %ld mismatches\n", bad);
  return bad != 0;
}
#endif
