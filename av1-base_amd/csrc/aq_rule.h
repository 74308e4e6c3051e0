// aq_rule.h - the activity-adaptive quantisation rule (av1mi_params.cq_level bits 8-10: aq_strength), all
// integers, for host and device: scene_kernels.hip runs it per superblock and per frame, tests/host/aq_rule_host.cpp compiles it
// for the CPU against the numpy restatement (tests/aq_ref.py).  Non-normative: the decoder only sees the per-superblock quantiser
// index (delta_q_present = 1, delta_q_res = 2).
//
//   8x8 unit     S, Q = sum and sum of squares of its 64 source luma samples (coded size: edge-extended to multiples of 8)
//                V = 64 Q - S^2,  v = V >> (12 + 2 (bit_depth - 8))  (the variance at 8-bit scale, floored),  e = L(v + 1)
//   L(x), x >= 1 k = floor(log2 x),  L = 16 k + (((x << 4) >> k) & 15): log2 in sixteenths, linear between powers of two
//   superblock   E = (sum e + n / 2) / n over its n units inside the coded frame
//   frame        M = (sum E + N / 2) / N over its N superblocks
//   delta        t = strength (E - M),  d = sign(t) ((|t| + 16) >> 5),  clamped to [max(-6, -((base - 1) / 4)), min(6, (255 - base) / 4)]
//   index        base_q_idx + 4 d   - at most 13 distinct values per frame, never outside 1 .. 255
#ifndef AV1MI_AQ_RULE_H
#define AV1MI_AQ_RULE_H
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_AQ_HD __host__ __device__
#else
#define AV1MI_AQ_HD
#endif

#define AV1MI_AQ_MAX_STRENGTH 4
#define AV1MI_AQ_MAX_DELTA 6    /* |d|: the index moves by at most 24 either way */

AV1MI_AQ_HD constexpr int av1mi_aq_log2_q4(uint32_t x) {
  const int k = 31 - __builtin_clz(x);
  return 16 * k + (int)((((uint64_t)x << 4) >> k) & 15);
}
// e of one 8x8 unit from its sum and sum of squares
AV1MI_AQ_HD inline int av1mi_aq_unit_energy(uint32_t S, uint32_t Q, int bit_depth) {
  const uint64_t V = 64ull * Q - (uint64_t)S * S;
  return av1mi_aq_log2_q4((uint32_t)(V >> (12 + 2 * (bit_depth - 8))) + 1u);
}
// rounded mean: E of a superblock from the sum over its n units, M of a frame from the sum over its N superblocks
AV1MI_AQ_HD inline int av1mi_aq_mean(uint32_t sum, uint32_t n) { return (int)((sum + n / 2) / n); }
// d of a superblock from its t, clamped so that base + 4 d stays inside 1 .. 255 (tpl_rule.h adds its term to t and comes here too)
AV1MI_AQ_HD inline int av1mi_aq_delta_of(int t, int base) {
  const int a = ((t < 0 ? -t : t) + 16) >> 5;
  int d = t < 0 ? -a : a;
  int lo = -((base - 1) / 4), hi = (255 - base) / 4;
  lo = lo < -AV1MI_AQ_MAX_DELTA ? -AV1MI_AQ_MAX_DELTA : lo;
  hi = hi > AV1MI_AQ_MAX_DELTA ? AV1MI_AQ_MAX_DELTA : hi;
  d = d < lo ? lo : (d > hi ? hi : d);
  return d;
}
AV1MI_AQ_HD inline int av1mi_aq_delta(int strength, int E, int M, int base) { return av1mi_aq_delta_of(strength * (E - M), base); }
AV1MI_AQ_HD inline int av1mi_aq_qindex_of(int strength, int E, int M, int base) { return base + 4 * av1mi_aq_delta(strength, E, M, base); }

#endif
