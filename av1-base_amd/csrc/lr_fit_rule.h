// lr_fit_rule.h - the self-guided restoration fit (av1mi_params.enable_lr bit 8, AV1MI_LR_FIT), all integers, for
// host and device: lr_fit_kernel.hip runs it per restoration unit, av1mi_syntax.cpp builds the fixed candidates' bit strings with its
// writers from its candidate tables (the restoration kernels' too, lr_pieces.h), tests/host/lr_fit_rule_host.cpp compiles it for the CPU against the numpy restatement (tests/sgr_fit_ref.py).
// Non-normative except for the syntax: the decoder sees lr_sgr_set and the weights (§5.11.58).
//
//   set t        radii and strengths (r0, eps0, r1, eps1) = Sgr_Params[t] (§7.17.3); r0 is 2 or 0, r1 is 1 or 0
//   sample       u = cdef << 4,  f0 = flt0 - u (0 when r0 = 0),  f1 = flt1 - u (0 when r1 = 0),  s = (src << 4) - u
//   unit         H00 = sum f0^2, H01 = sum f0 f1, H11 = sum f1^2, C0 = sum f0 s, C1 = sum f1 s   (exact, |sum| < 2^42)
//   normalise    k = max(0, bitlength(max |sum|) - 26), every sum >> k (arithmetic)
//   rdiv(a, b)   sign(a) ((|a| + (b >> 1)) / b), b > 0
//   both radii   det = H00 H11 - H01^2 (absent if <= 0); x0 = rdiv(128 (C0 H11 - C1 H01), det), x1 = rdiv(128 (C1 H00 - C0 H01), det)
//                w = 128 - x0 - x1, xqd1 = clamp(w, -32, 95); if the clamp acted: T = 128 - xqd1, D = H00 - 2 H01 + H11 and, if D > 0,
//                x0 = rdiv(128 (C0 - C1) - T (H01 - H11), D);  xqd0 = clamp(x0, -96, 31)
//   r1 = 0       absent if H00 <= 0; xqd0 = clamp(rdiv(128 C0, H00), -96, 31), xqd1 = clamp(128 - xqd0, -32, 95) (implied, not coded)
//   r0 = 0       absent if H11 <= 0; xqd0 = 0 (not coded), xqd1 = clamp(128 - rdiv(128 C1, H11), -32, 95)
#ifndef AV1MI_LR_FIT_RULE_H
#define AV1MI_LR_FIT_RULE_H
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_FIT_HD __host__ __device__
#else
#define AV1MI_FIT_HD
#endif

#define AV1MI_LR_FIT_SETS 16
#define AV1MI_LR_FIT_CANDS 23   /* off, 3 Wiener, 3 fixed self-guided, 16 fitted sets */
#define AV1MI_SGR_XQD0_MIN (-96)
#define AV1MI_SGR_XQD0_MAX 31
#define AV1MI_SGR_XQD1_MIN (-32)
#define AV1MI_SGR_XQD1_MAX 95

// Sgr_Params (§7.17.3): { r0, eps0, r1, eps1 } =
//   {2,12,1,4} {2,15,1,6} {2,18,1,8} {2,21,1,9} {2,24,1,10} {2,29,1,11} {2,36,1,12} {2,45,1,13} {2,56,1,14} {2,68,1,15}
//   {0,0,1,5} {0,0,1,8} {0,0,1,11} {0,0,1,14} {2,30,0,0} {2,75,0,0}
// (packed, so that host and device read the same constants without a table in memory)
AV1MI_FIT_HD constexpr int av1mi_sgr_r0(int t) { return t < 10 || t >= 14 ? 2 : 0; }
AV1MI_FIT_HD constexpr int av1mi_sgr_r1(int t) { return t < 14 ? 1 : 0; }
AV1MI_FIT_HD constexpr int av1mi_sgr_eps0(int t) {   // a byte per set
  const uint64_t lo = 0x2D241D1815120F0Cull /* sets 7 .. 0 */, hi = 0x4B1E000000004438ull /* sets 15 .. 8 */;
  return (int)(((t < 8 ? lo : hi) >> (8 * (t & 7))) & 255);
}
AV1MI_FIT_HD constexpr int av1mi_sgr_eps1(int t) { return (int)((0x00EB85FEDCBA9864ull >> (4 * t)) & 15); }   // a nibble per set

// ---- the fixed candidates (restated in oracle/av1o_lr.c av1o_wiener_candidates / av1o_sgr_candidates): initialisers,
// for the kernels' __constant__ copies (lr_pieces.h) and the host's tables below (the fixed candidates' bit strings, av1mi_syntax.cpp)
#define AV1MI_WIENER_CAND { { 0, 0, -4 }, { 1, -3, -6 }, { 3, -7, 15 } }       /* taps 0 .. 2 of both passes */
#define AV1MI_WIENER_CAND_UV { { 0, 0, -4 }, { 0, 0, 16 }, { 0, 6, 20 } }      /* chroma (enable_lr 3 / 4): tap 0 is 0 and not coded, §5.11.58 */
#define AV1MI_SGR_CAND { { 9, 31, 31 }, { 9, 0, 31 }, { 9, 31, 95 } }          /* { lr_sgr_set, xqd0, xqd1 } */
#define AV1MI_SGR_CAND_SET 9   /* the set of every fixed self-guided candidate: both radii non-zero */
const int8_t av1mi_wiener_cand[3][3] = AV1MI_WIENER_CAND, av1mi_wiener_cand_uv[3][3] = AV1MI_WIENER_CAND_UV, av1mi_sgr_cand[3][3] = AV1MI_SGR_CAND;

AV1MI_FIT_HD inline int av1mi_fit_clamp(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
AV1MI_FIT_HD inline long long av1mi_fit_rdiv(long long a, long long b) {
  const long long q = ((a < 0 ? -a : a) + (b >> 1)) / b;
  return a < 0 ? -q : q;
}

// The weights of set t from the unit's sums { H00, H01, H11, C0, C1 }; returns 0 if the candidate is absent
AV1MI_FIT_HD inline int av1mi_lr_fit_solve(int t, const long long *sums, int *xqd0, int *xqd1) {
  unsigned long long m = 0;
  for (int i = 0; i < 5; i++) { const unsigned long long a = (unsigned long long)(sums[i] < 0 ? -sums[i] : sums[i]); m = a > m ? a : m; }
  int bl = 0;
  while (m >> bl) bl++;
  const int k = bl > 26 ? bl - 26 : 0;
  const long long H00 = sums[0] >> k, H01 = sums[1] >> k, H11 = sums[2] >> k, C0 = sums[3] >> k, C1 = sums[4] >> k;
  const int r0 = av1mi_sgr_r0(t), r1 = av1mi_sgr_r1(t);
  *xqd0 = 0; *xqd1 = 0;
  if (r0 && r1) {
    const long long det = H00 * H11 - H01 * H01;
    if (det <= 0) return 0;
    long long x0 = av1mi_fit_rdiv(128 * (C0 * H11 - C1 * H01), det);
    const long long x1 = av1mi_fit_rdiv(128 * (C1 * H00 - C0 * H01), det);
    const long long w = 128 - x0 - x1;
    *xqd1 = av1mi_fit_clamp(w, AV1MI_SGR_XQD1_MIN, AV1MI_SGR_XQD1_MAX);
    if (*xqd1 != w) {   // refit x0 on the line x0 + x1 = T
      const long long T = 128 - *xqd1, D = H00 - 2 * H01 + H11;
      if (D > 0) x0 = av1mi_fit_rdiv(128 * (C0 - C1) - T * (H01 - H11), D);
    }
    *xqd0 = av1mi_fit_clamp(x0, AV1MI_SGR_XQD0_MIN, AV1MI_SGR_XQD0_MAX);
    return 1;
  }
  if (r0) {   // r1 = 0: sets 14, 15
    if (H00 <= 0) return 0;
    *xqd0 = av1mi_fit_clamp(av1mi_fit_rdiv(128 * C0, H00), AV1MI_SGR_XQD0_MIN, AV1MI_SGR_XQD0_MAX);
    *xqd1 = av1mi_fit_clamp(128 - *xqd0, AV1MI_SGR_XQD1_MIN, AV1MI_SGR_XQD1_MAX);
    return 1;
  }
  if (H11 <= 0) return 0;   // r0 = 0: sets 10 .. 13
  *xqd1 = av1mi_fit_clamp(128 - av1mi_fit_rdiv(128 * C1, H11), AV1MI_SGR_XQD1_MIN, AV1MI_SGR_XQD1_MAX);
  return 1;
}

// ---- loop restoration unit syntax (§5.11.58): literal bits, MSB first in the low `len` bits.  Mirrors
// decode_signed_subexp_with_ref_bool / decode_subexp_bool / NS / inverse_recenter.  The writers take any sink with put(value, bits):
// the bit string, or the count alone (lr_rate_rule.h weighs a unit's length).
struct Av1miBitString {
  unsigned long long bits = 0;
  int len = 0;
  AV1MI_FIT_HD void put(unsigned v, int n) { for (int i = n - 1; i >= 0; i--) { bits = (bits << 1) | ((v >> i) & 1); len++; } }
};
struct Av1miBitCount {
  int len = 0;
  AV1MI_FIT_HD void put(unsigned, int n) { len += n; }
};
template <typename SINK>
AV1MI_FIT_HD inline void lr_put_ns(SINK &b, int n, int v) {
  int w = 0, x = n;
  while (x) { w++; x >>= 1; }
  const int m = (1 << w) - n;
  if (v < m) b.put((unsigned)v, w - 1);
  else { const int extra = v + m; b.put((unsigned)(extra >> 1), w - 1); b.put((unsigned)(extra & 1), 1); }
}
template <typename SINK>
AV1MI_FIT_HD inline void lr_put_subexp(SINK &b, int num_syms, int k, int v) {
  int i = 0, mk = 0;
  for (;;) {
    const int b2 = i ? k + i - 1 : k, a = 1 << b2;
    if (num_syms <= mk + 3 * a) { lr_put_ns(b, num_syms - mk, v - mk); return; }
    if (v >= mk + a) { b.put(1, 1); i++; mk += a; }
    else { b.put(0, 1); b.put((unsigned)(v - mk), b2); return; }
  }
}
AV1MI_FIT_HD inline int lr_recenter(int r, int v) { return v > 2 * r ? v : (v >= r ? (v - r) << 1 : ((r - v) << 1) - 1); }
template <typename SINK>
AV1MI_FIT_HD inline void lr_put_signed_ref(SINK &b, int low, int high, int k, int r, int v) {
  const int mx = high - low, x = v - low, rr = r - low;
  if ((rr << 1) <= mx) lr_put_subexp(b, mx, k, lr_recenter(rr, x));
  else lr_put_subexp(b, mx, k, lr_recenter(mx - 1 - rr, mx - 1 - x));
}

// A self-guided unit: lr_sgr_set L(4), then the weight(s) whose radius is non-zero against the plane's RefSgrXqd (ref0, ref1), k = 4:
// at most 4 + 9 + 9 = 22 bits.  The caller carries the reference: after the unit it is (xqd0, xqd1), implied values included.
template <typename SINK>
AV1MI_FIT_HD inline void av1mi_lr_sgr_put(SINK &b, int set, int xqd0, int xqd1, int ref0, int ref1) {
  b.put((unsigned)set, 4);
  if (av1mi_sgr_r0(set)) lr_put_signed_ref(b, AV1MI_SGR_XQD0_MIN, AV1MI_SGR_XQD0_MAX + 1, 4, ref0, xqd0);
  if (av1mi_sgr_r1(set)) lr_put_signed_ref(b, AV1MI_SGR_XQD1_MIN, AV1MI_SGR_XQD1_MAX + 1, 4, ref1, xqd1);
}
AV1MI_FIT_HD inline Av1miBitString av1mi_lr_sgr_code(int set, int xqd0, int xqd1, int ref0, int ref1) {
  Av1miBitString b;
  av1mi_lr_sgr_put(b, set, xqd0, xqd1, ref0, ref1);
  return b;
}

#endif
