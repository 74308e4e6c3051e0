// quant_pieces.h - the quantiser rule of the reconstruction kernel (recon_kernel.hip; DESIGN.md §3.5, AV1 spec §7.12.3), for host and
// device like intra_pieces.h / aq_rule.h: tests/host/quant_pieces_host.cpp compiles it for the CPU against the oracle's quantiser
// (oracle/av1o_enc.c, code_tx_block).
//
//   dead zone   class of coefficient (row, col) in a coded area of width cw: 0 where row + col < cw / 4, 1 below cw / 2, else 2;
//               rounding term 3 q / 8, q / 4, q / 8 of the position's step q
//   level       min((((|v| << TSH) + rnd) * recip) >> 32, 0x7FFF) with the sign of v;  recip = ceil(2^32 / q),  TSH = 0 / 1 / 2 for
//               transforms up to 16 / of 32 / of 64 points (the dequantiser's shift of the size class)
//   dequantiser ((level * q) & 0xFFFFFF) >> TSH with the sign, clamped to [-2^(7 + bd), 2^(7 + bd) - 1]   (normative)
//   scan        by anti-diagonal d = row + col, odd ones by increasing row, even ones by increasing column: key = d << 6 | position.
//               A lane that holds one row (one column) of the block has its largest key at its last nonzero column (row): with the
//               other coordinate fixed the anti-diagonal grows with it.  So the loops - flat or with quantiser matrices: the argument
//               does not involve the step - track that one index and derive key and extent once from it.
#ifndef AV1MI_QUANT_PIECES_H
#define AV1MI_QUANT_PIECES_H
#include <stdint.h>

#ifdef __HIPCC__
#define AV1MI_QUANT_FN static __host__ __device__ __forceinline__
#else
#define AV1MI_QUANT_FN static inline
#endif

namespace av1mi_quant {

enum { LEVEL_CAP = 0x7FFF };

AV1MI_QUANT_FN uint32_t q_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// dead-zone class of a position, and the rounding term of a class
AV1MI_QUANT_FN int dz_class(int row, int col, int cw) { const int d = row + col; return d < (cw >> 2) ? 0 : (d < (cw >> 1) ? 1 : 2); }
AV1MI_QUANT_FN uint32_t dz_round(uint32_t q, int cls) { return cls == 0 ? (3 * q) >> 3 : (cls == 1 ? q >> 2 : q >> 3); }

// the per-lane form of the class: a lane whose positions share one coordinate `fixed` and run over the other, t = 0, 1, ..., is in
// class 0 while t < dz_ta, in class 1 while t < dz_tb, then in class 2
AV1MI_QUANT_FN int dz_ta(int fixed, int cw) { return (cw >> 2) - fixed; }
AV1MI_QUANT_FN int dz_tb(int fixed, int cw) { return (cw >> 1) - fixed; }
AV1MI_QUANT_FN uint32_t dz_pick(int t, int ta, int tb, uint32_t r0, uint32_t r1, uint32_t r2) { return t < ta ? r0 : (t < tb ? r1 : r2); }

// ... with the index a compile-time constant of an unrolled loop, most compares fold away.  A lane that holds one ROW of a coded area of
// width CW (the butterfly path; t = column j, fixed = row): columns from CW / 2 on are in class 2 in every row, those from CW / 4 on
// never in class 0
template <int CW>
AV1MI_QUANT_FN uint32_t dz_round_row(int j, int ta, int tb, uint32_t r0, uint32_t r1, uint32_t r2) {
  return j >= (CW >> 1) ? r2 : (j >= (CW >> 2) ? (j < tb ? r1 : r2) : dz_pick(j, ta, tb, r0, r1, r2));
}
// A lane of the matrix-core quantiser (32x32): column on the lane, rows k = mm_row(reg, mh); thresholds ta / tb for fixed = column + 4 mh,
// t = (reg & 3) + 8 (reg >> 2).  Registers 8 .. 15 (k >= 16) are in class 2, registers 4 .. 7 (k >= 8) never in class 0
AV1MI_QUANT_FN int mm_row(int reg, int mh) { return (reg & 3) + 8 * (reg >> 2) + 4 * mh; }
AV1MI_QUANT_FN uint32_t dz_round_mm(int reg, int ta, int tb, uint32_t r0, uint32_t r1, uint32_t r2) {
  return reg >= 8 ? r2 : (reg >= 4 ? ((reg & 3) + 8 < tb ? r1 : r2) : dz_pick(reg, ta, tb, r0, r1, r2));
}

// sign mask of a coefficient (0 or -1) and its magnitude; a magnitude back under that mask
AV1MI_QUANT_FN int sign_mask(int v) { return v >> 31; }
AV1MI_QUANT_FN uint32_t magnitude(int v, int sgn) { return (uint32_t)((v ^ sgn) - sgn); }
AV1MI_QUANT_FN int with_sign(uint32_t m, int sgn) { return ((int)m ^ sgn) - sgn; }

// the level's magnitude from the coefficient's; rnd = dz_round(q, class)
template <int TSH>
AV1MI_QUANT_FN uint32_t level_abs(uint32_t av, uint32_t rnd, uint32_t recip) {
  const uint32_t lv = q_mulhi((av << TSH) + rnd, recip);
  return lv > LEVEL_CAP ? (uint32_t)LEVEL_CAP : lv;
}

// level * step for the dequantiser: both are below 2^24, which is all the two forms need to agree.  level <= 0x7FFF; the step of the
// flat quantiser is below 2^13 (ac_q at most 1828 at 8 bit, 7312 at 10), and a quantiser-matrix step Round2(q * Quantizer_Matrix, 5) with
// matrix entries of 30 .. 242 is at most 13 824 at 8 bit and 55 297 at 10 - below 2^16 (tests/host/quant_pieces_host.cpp derives the bound
// from the tables).  The device library's __umul24 is plain C, and with the step's range unknown to the compiler it ends in v_mul_lo_u32
// here (8 per chroma pair, behind `if (lv)`), not in the 24-bit multiply its name promises
AV1MI_QUANT_FN uint32_t q_mul24(uint32_t lv, uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(lv, q);
#else
  return lv * q;
#endif
}

// the normative dequantiser; lim = 1 << (7 + bit depth)
template <int TSH>
AV1MI_QUANT_FN int dequant(uint32_t lv, uint32_t q, int sgn, int lim) {
  int d = (int)((q_mul24(lv, q) & 0xFFFFFFu) >> TSH);
  d = with_sign((uint32_t)d, sgn);
  return d < -lim ? -lim : (d > lim - 1 ? lim - 1 : d);
}

// ---- the quantiser step of one coefficient: what every quantiser loop of the kernel calls.  mag = the level's magnitude (nonzero: the
// position counts for the scan key and the extent), level = it with the coefficient's sign (what goes to the level buffer), deq = the
// dequantised value the inverse transform takes
struct Quantised { uint32_t mag; int level, deq; };
// coefficient -> level, given the position's rounding term and reciprocal
template <int TSH>
AV1MI_QUANT_FN Quantised quantise(int v, uint32_t rnd, uint32_t recip) {
  const int sgn = sign_mask(v);
  const uint32_t lv = level_abs<TSH>(magnitude(v, sgn), rnd, recip);
  return Quantised{ lv, with_sign(lv, sgn), 0 };
}
// coefficient -> level and dequantised value, given the position's (q, recip, rnd).  The dequantiser stays behind `if (mag)`: a column
// with no level in any row costs the wave nothing
template <int TSH>
AV1MI_QUANT_FN Quantised quantise_dequantise(int v, uint32_t q, uint32_t recip, uint32_t rnd, int lim) {
  Quantised z = quantise<TSH>(v, rnd, recip);
  if (z.mag) z.deq = dequant<TSH>(z.mag, q, sign_mask(v), lim);
  return z;
}
// a stored level -> dequantised value
template <int TSH>
AV1MI_QUANT_FN int dequant_level(int level, uint32_t q, int lim) { const int sgn = sign_mask(level); return dequant<TSH>(magnitude(level, sgn), q, sgn, lim); }

// scan key of the position (the larger, the later in scan order) and its extent {row + 1, column + 1} as packed 16-bit values
AV1MI_QUANT_FN int scan_key(int row, int col) { const int d = row + col; return (d << 6) | ((d & 1) ? row : col); }
AV1MI_QUANT_FN uint32_t extent(int row, int col) { return ((uint32_t)(row + 1) << 16) | (uint32_t)(col + 1); }
// index of the position in the default zig-zag scan of an n x n block: the positions on the anti-diagonals before its
// own, then its place on that one (odd anti-diagonals run with increasing row, even ones with increasing column)
AV1MI_QUANT_FN constexpr int scan_index(int row, int col, int n) {
  const int d = row + col;
  const int before = d < n ? (d * (d + 1)) >> 1 : n * n - (((2 * n - 1 - d) * (2 * n - d)) >> 1);
  const int lo = d - (n - 1) > 0 ? d - (n - 1) : 0;
  return before + ((d & 1) ? row - lo : col - lo);
}

}  // namespace av1mi_quant
#endif
