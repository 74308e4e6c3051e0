// lr_rate_rule.h - the rate term of the loop-restoration unit decisions (av1mi_params.enable_lr bits 14 and 15, AV1MI_LR_RD; DESIGN.md
// §3 item 9g), all integers, for host and device: the three restoration kernels weigh a candidate's side information against its error
// with it, av1mi_syntax.cpp derives lambda and av1mi_ctx.cpp reports the bits (av1mi_lr_rd_result), tests/host/lr_rate_rule_host.cpp compiles it for the
// CPU against the numpy restatement (tests/lr_rd_ref.py).  Non-normative: the decoder sees the units' types and coefficients as ever.
//
//   lambda       q = the dc step of base_q_idx at the stream's bit depth, lambda0 = (13 q^2) >> 9 (libaom's RDCOST weighs D << 7 against
//                rate x rdmult, rdmult about 3.3 q^2: a bit is worth 3.3 q^2 / 128 squared-error units); scale s = 0 .. 3:
//                lambda0, lambda0 >> 1, lambda0 >> 2, lambda0 << 1, at least 1
//   T16(p)       240 - L(p): the cost in sixteenths of a bit of a symbol of probability p / 32768, L = aq_rule.h's log2 in sixteenths;
//                the restoration type from the default CDFs, no adaptation
//   Lc(c)        the length of the candidate's coefficients (§5.11.58) against the plane's tile-start references: 0 for off
//   B16(c)       16 Lc(c) + T16(type of c)
//   J(c)         16 D(c) + lambda B16(c), D the candidate's exact SSE (16 D < 2^42, lambda B16 < 2^32)
// A unit takes the first minimum of J over its present candidates 0 .. 22; the fitted Wiener filter (23) replaces that winner iff its J
// is strictly smaller.  lambda = 0 is the mode off: the order of 16 D is that of D.
#ifndef AV1MI_LR_RATE_RULE_H
#define AV1MI_LR_RATE_RULE_H
#include "aq_rule.h"           // L
#include "wiener_fit_rule.h"   // and lr_fit_rule.h: the syntax writers

// av1_default_switchable_restore_cdf and av1_default_use_wiener_cdf (av1_tables.h, whose arrays are no constant expressions; the host
// program checks these against them)
#define AV1MI_LR_CDF_SWITCHABLE_0 9413
#define AV1MI_LR_CDF_SWITCHABLE_1 22581
#define AV1MI_LR_CDF_USE_WIENER 11570

AV1MI_FIT_HD constexpr int av1mi_lr_t16(uint32_t p) { return 240 - av1mi_aq_log2_q4(p); }
// the type symbol of a unit - type: 0 = NONE, 1 = WIENER, 2 = SGRPROJ - on a switchable plane, or off / on on a Wiener-only one
AV1MI_FIT_HD constexpr int av1mi_lr_type_t16(int switchable, int type) {
  return switchable ? (type == 0 ? av1mi_lr_t16(AV1MI_LR_CDF_SWITCHABLE_0)
                                 : (type == 1 ? av1mi_lr_t16(AV1MI_LR_CDF_SWITCHABLE_1 - AV1MI_LR_CDF_SWITCHABLE_0) : av1mi_lr_t16(32768 - AV1MI_LR_CDF_SWITCHABLE_1)))
                    : (type == 0 ? av1mi_lr_t16(AV1MI_LR_CDF_USE_WIENER) : av1mi_lr_t16(32768 - AV1MI_LR_CDF_USE_WIENER));
}
// the type of choice c (0 .. 23, av1mi_lr_wiener_fit_result's numbering)
AV1MI_FIT_HD constexpr int av1mi_lr_choice_type(int c) { return c == 0 ? 0 : (c <= 3 || c == AV1MI_LR_WFIT_CHOICE ? 1 : 2); }

// Lc of a Wiener filter with the vertical taps (v0, v1, v2) and the horizontal (h0, h1, h2) - what av1mi_lr_wiener_code writes against
// Wiener_Taps_Mid in both passes; first = 1 for chroma, whose tap 0 is not coded - and of a self-guided unit against Sgrproj_Xqd_Mid.
// (Scalars and the counting sink: a kernel calls these per unit without arrays of its own.)
AV1MI_FIT_HD inline int av1mi_lr_wiener_lc(int first, int v0, int v1, int v2, int h0, int h1, int h2) {
  Av1miBitCount b;
  if (!first) lr_put_signed_ref(b, av1mi_wiener_tap_min(0), av1mi_wiener_tap_max(0) + 1, 1, av1mi_wiener_tap_mid(0), v0);
  lr_put_signed_ref(b, av1mi_wiener_tap_min(1), av1mi_wiener_tap_max(1) + 1, 2, av1mi_wiener_tap_mid(1), v1);
  lr_put_signed_ref(b, av1mi_wiener_tap_min(2), av1mi_wiener_tap_max(2) + 1, 3, av1mi_wiener_tap_mid(2), v2);
  if (!first) lr_put_signed_ref(b, av1mi_wiener_tap_min(0), av1mi_wiener_tap_max(0) + 1, 1, av1mi_wiener_tap_mid(0), h0);
  lr_put_signed_ref(b, av1mi_wiener_tap_min(1), av1mi_wiener_tap_max(1) + 1, 2, av1mi_wiener_tap_mid(1), h1);
  lr_put_signed_ref(b, av1mi_wiener_tap_min(2), av1mi_wiener_tap_max(2) + 1, 3, av1mi_wiener_tap_mid(2), h2);
  return b.len;
}
AV1MI_FIT_HD inline int av1mi_lr_sgr_lc(int set, int xqd0, int xqd1) {
  Av1miBitCount b;
  av1mi_lr_sgr_put(b, set, xqd0, xqd1, -32, 31);
  return b.len;
}

AV1MI_FIT_HD constexpr int av1mi_lr_b16(int lc, int t16) { return 16 * lc + t16; }
AV1MI_FIT_HD constexpr unsigned long long av1mi_lr_j(unsigned long long d, unsigned long long lambda, int b16) { return 16 * d + lambda * (unsigned long long)b16; }

// lambda from the dc step (av1_dc_q8 / av1_dc_q10 of base_q_idx) and the scale s
AV1MI_FIT_HD constexpr unsigned long long av1mi_lr_lambda_of_step(unsigned long long q, int s) {
  const unsigned long long l0 = (13 * q * q) >> 9, l = s == 0 ? l0 : (s == 1 ? l0 >> 1 : (s == 2 ? l0 >> 2 : l0 << 1));
  return l < 1 ? 1 : l;
}

#endif
