// ssim_rule.h - the structural-similarity rule of the quality pass (include/av1mi.h: av1mi_quality), all integers,
// for host and device: quality_kernel.hip runs it per window, tests/host/ssim_rule_host.cpp compiles it for the CPU against the numpy
// restatement (tests/ssim_ref.py).  The geometry and constants are libaom's aom_ssim2 / similarity(); every window value is truncated
// to Q24, so every implementation agrees bit for bit.
//
//   planes       a = the reference, b = the test plane, h x w samples at the signalled size (chroma (h + 1) / 2 x (w + 1) / 2)
//   windows      8 x 8 at (4 i, 4 j), i = 0 .. ny - 1, ny = (h - 8) / 4 + 1 for h >= 8, else 0; nx likewise from w
//   sums         over a window's 64 samples: s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum a b
//   constants    C1 = 64^2 (0.01 L)^2, C2 = 64^2 (0.03 L)^2 as libaom rounds them: 26634, 239708 at 8 bits, 428658, 3857925 at 10
//   factors      A = 2 s1 s2 + C1,  B = s1^2 + s2^2 + C1,  Cn = 2 (64 s12 - s1 s2) + C2 (signed),  D = 64 ss - s1^2 - s2^2 + C2
//                0 < A <= B < 2^34 and |Cn| <= D < 2^35 (the mean and Cauchy-Schwarz inequalities): every product below is under 2^59
//   value        l = (A << 24) / B,  c = (|Cn| << 24) / D,  v = (l c) >> 24,  w = Cn < 0 ? -v : v   - in [-2^24, 2^24]
//   plane        ssim_sum = sum w (int64), windows = ny nx, sse = sum (a - b)^2 over the whole plane (uint64); the value a person
//                reads, ssim_sum / (windows 2^24), is formed on the host by whoever wants it
#ifndef AV1MI_SSIM_RULE_H
#define AV1MI_SSIM_RULE_H
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_SSIM_HD __host__ __device__
#else
#define AV1MI_SSIM_HD
#endif

#define AV1MI_SSIM_Q 24   /* a window's value is a Q24 number */

AV1MI_SSIM_HD constexpr uint32_t av1mi_ssim_c1(int bit_depth) { return bit_depth > 8 ? 428658u : 26634u; }
AV1MI_SSIM_HD constexpr uint32_t av1mi_ssim_c2(int bit_depth) { return bit_depth > 8 ? 3857925u : 239708u; }
// windows along a dimension of n samples
AV1MI_SSIM_HD constexpr int av1mi_ssim_windows(int n) { return n >= 8 ? (n - 8) / 4 + 1 : 0; }

// the four factors of a window from its sums
struct Av1miSsimFactors { uint64_t A, B, D; int64_t Cn; };
AV1MI_SSIM_HD inline Av1miSsimFactors av1mi_ssim_factors(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12, int bit_depth) {
  const uint64_t p = (uint64_t)s1 * s2, q = (uint64_t)s1 * s1 + (uint64_t)s2 * s2;
  const uint64_t c1 = av1mi_ssim_c1(bit_depth), c2 = av1mi_ssim_c2(bit_depth);
  Av1miSsimFactors F;
  F.A = 2 * p + c1;
  F.B = q + c1;
  F.Cn = 2 * ((int64_t)(64ull * s12) - (int64_t)p) + (int64_t)c2;
  F.D = 64ull * ss - q + c2;
  return F;
}
// w of a window from its sums
AV1MI_SSIM_HD inline int32_t av1mi_ssim_window(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12, int bit_depth) {
  const Av1miSsimFactors F = av1mi_ssim_factors(s1, s2, ss, s12, bit_depth);
  const uint64_t l = (F.A << AV1MI_SSIM_Q) / F.B;
  const uint64_t c = ((uint64_t)(F.Cn < 0 ? -F.Cn : F.Cn) << AV1MI_SSIM_Q) / F.D;
  const int32_t v = (int32_t)((l * c) >> AV1MI_SSIM_Q);
  return F.Cn < 0 ? -v : v;
}

#endif
