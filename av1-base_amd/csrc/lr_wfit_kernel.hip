// lr_wfit_kernel.hip - the Wiener restoration fit (av1mi_params.enable_lr bit 10, AV1MI_LR_WIENER_FIT): per
// restoration unit six taps by least squares - three of the vertical pass, three of the horizontal (wiener_fit_rule.h) - the exact SSE
// of the fitted filter, the override of units it improves, and every Wiener unit's bit string for symbolize.
//
// Replaces the Wiener coefficient search of the SVT-AV1 worker behind `run_av1an`.  Normative part: §7.17.4 (horizontal pass with the
// taps of pass 1, Round2 by 3, clamp; vertical pass with the taps of pass 0, Round2 by 11), §7.17.6 (stripes) and §5.11.58 (the taps
// against RefLrWiener).
//
// MI355X mapping: lr_kernel.hip's - one 64-lane wave per 16-row slice of a luma unit or of a pair of chroma units, lane = column, the
// same grid, the window and the Wiener tile in LDS (6.2 KB per wave + 64 bytes of the units' taps).  It runs after the decision over
// the other candidates has been taken and applied (lr_kernel.hip, or lr_fit_kernel.hip with the self-guided fit), in four launches:
//   1 sums      the 27 sums per lane over the section's rows (32-bit: |D| <= 2046, 16 rows: < 2^27), reduced per half wave, one 64-bit
//               atomic per sum and half into the unit's sums (a unit of 256 has at most 383 x 391 samples: |sum| < 2^40)
//   2 SSE       every slice solves its units' taps from the complete sums (lanes 0 and 1, one unit each), filters with the two tap
//               arrays and adds its exact SSE; the unit's first lane records the taps
//   3 override  a unit whose fitted error - with the rate term, its J - is strictly below its winner's is filtered again with the fitted
//               taps (read-only on every table: the slices of a unit take the same decision)
//   4 codes     one thread per (frame, plane, tile) walks the tile's units in coding order: the final choice (23 = fitted) into the
//               record and the choice table, and the bits of every Wiener unit against the carried RefLrWiener
#include <hip/hip_runtime.h>
#include <type_traits>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "wiener_fit_rule.h"
#include "lr_rate_rule.h"

namespace {

#include "lr_pieces.h"

__shared__ int g_wtap[2][8];   // [unit of the wave's section]: present, cv0 .. cv2, ch0 .. ch2

// where a unit's winner's error is: the self-guided fit's table when it ran, else lr_kernel.hip's sums
struct BaseErr {
  const uint8_t *choice;                // [frame][restored plane][unit]
  const unsigned long long *unit_sse;   // likewise, 8 per unit
  const unsigned long long *fit_err;    // [frame][plane 0..2][unit][23], or null
  const int8_t *fit_rec;                // with fit_err: the self-guided fit's records [4] and codes [2], which phase 4 writes again
  uint32_t *fit_code;
};
__device__ __forceinline__ unsigned long long base_err_of(const BaseErr &B, size_t sse_idx, size_t fit_idx) {
  const int c = B.choice[sse_idx];
  return B.fit_err ? B.fit_err[fit_idx * AV1MI_LR_FIT_CANDS + c] : B.unit_sse[sse_idx * 8 + c];
}

// Does the fitted filter of unit u (present; cu: the unit in the fixed candidates' tables; sub: a chroma plane) replace the unit's winner:
// iff its error is strictly smaller or, with the rate term, its J = 16 D + lambda B16 is (lr_rate_rule.h).  The winner's coefficient
// length is the host's against the tile-start reference for a fixed candidate, the syntax writer's for fitted weights and taps.
__device__ __forceinline__ bool wfit_overrides(const Av1miDevParams &P, const BaseErr &B, const Av1miLrWfit &F, size_t cu, size_t u, int sub) {
  const unsigned long long ef = F.err[u], eb = base_err_of(B, cu, u);
  if (!P.lr_lambda) return ef < eb;
  const int sw = P.enable_lr == 2, c = B.choice[cu];
  int lc = 0;
  if (c >= 7) { const int8_t *q = B.fit_rec + u * 4; lc = av1mi_lr_sgr_lc(q[1], q[2], q[3]); }
  else if (c >= 4) lc = P.sgr_code_len[0][c - 4];
  else if (c) lc = sub ? P.lr_code_len_uv[0][c - 1] : P.lr_code_len[0][c - 1];
  const int8_t *r = F.rec + u * 8;
  const int bf = av1mi_lr_b16(av1mi_lr_wiener_lc(sub, r[2], r[3], r[4], r[5], r[6], r[7]), av1mi_lr_type_t16(sw, 1));
  return av1mi_lr_j(ef, P.lr_lambda, bf) < av1mi_lr_j(eb, P.lr_lambda, av1mi_lr_b16(lc, av1mi_lr_type_t16(sw, av1mi_lr_choice_type(c))));
}

// PHASE 1: sums; 2: solve and SSE; 3: override.  The grid is lr_unit_kernel's.
template <typename PIX, int PHASE>
__global__ void __launch_bounds__(64) lr_wfit_kernel(Av1miDevParams P, const PIX *__restrict__ pre, const PIX *__restrict__ cdef,
                                                    const PIX *__restrict__ src, PIX *__restrict__ out, BaseErr B, Av1miLrWfit F) {
  // the blocks are those of the cells (the units of lr_unit_shift 0); sums, taps, errors and records are those of the unit a cell lies in
  const int lane = threadIdx.x;
  const LrWave w = lr_wave(P, blockIdx.x);
  if (w.idle) return;
  pre += w.plane_off; cdef += w.plane_off; src += w.plane_off; out += w.plane_off;
  const int sub = w.sub, stride = w.stride, x1 = w.x1, y0 = w.y0, y1 = w.y1;
  const int maxv = (1 << P.bit_depth) - 1, bd = P.bit_depth;
  const size_t sse_base = w.sse_base, fit_base = w.fit_base;
  for (int xs = w.x0; xs < x1; xs += 64) {
    const int x = xs + lane;
    const bool active = x < x1;
    const LrSection u = lr_section(P, w, xs, lane);
    const int lo = u.lo, hi = u.hi, hsel = u.hsel, unit = u.unit;
    int fv[7], fh[7];
    bool mine = false, any = true;
    if constexpr (PHASE == 2) {
      __syncthreads();
      if (lane < 2) {
        int cv[3], ch[3];
        const int ok = av1mi_wiener_fit(F.sums + (fit_base + (lane ? hi : lo)) * AV1MI_LR_WFIT_SUMS, sub, cv, ch, nullptr);
        g_wtap[lane][0] = ok;
        for (int j = 0; j < 3; j++) { g_wtap[lane][1 + j] = ok ? cv[j] : 0; g_wtap[lane][4 + j] = ok ? ch[j] : 0; }
      }
      __syncthreads();
      mine = active && g_wtap[hsel][0] != 0;
      any = g_wtap[0][0] != 0 || g_wtap[1][0] != 0;
      taps7(g_wtap[hsel][1], g_wtap[hsel][2], g_wtap[hsel][3], fv); taps7(g_wtap[hsel][4], g_wtap[hsel][5], g_wtap[hsel][6], fh);
      if (lr_records(P, w, unit, x, active)) {   // the unit's record (present, taps); the choice follows in phase 4
        int8_t *r = F.rec + (fit_base + unit) * 8;
        for (int j = 0; j < 7; j++) r[1 + j] = (int8_t)g_wtap[hsel][j];
      }
    }
    if constexpr (PHASE == 3) {
      // both units' decisions in every lane: the stripe loop below stays uniform
      bool ov[2];
      for (int h = 0; h < 2; h++) {
        const size_t fu = fit_base + (h ? hi : lo);
        ov[h] = F.rec[fu * 8 + 1] != 0 && wfit_overrides(P, B, F, sse_base + (h ? hi : lo), fu, sub);
      }
      const int8_t *r = F.rec + (fit_base + unit) * 8;
      taps7(r[2], r[3], r[4], fv); taps7(r[5], r[6], r[7], fh);
      mine = active && ov[hsel];
      any = ov[0] || ov[1];
    }
    if (!any) continue;
    [[maybe_unused]] unsigned long long sse = 0;
    for (int st = lr_first_stripe(y0, sub); lr_stripe_row0(st, sub) < y1; st++) {
      const LrStripe S = lr_stripe(st, y0, y1, sub);
      const int ya = S.ya, yb = S.yb;
      __syncthreads();
      lr_stage<PIX>(cdef, pre, xs, ya, yb, S.s0, S.s1, w.W, w.H, stride, lane);
      __syncthreads();
      if constexpr (PHASE == 1) {
        int acc[AV1MI_LR_WFIT_SUMS];
#pragma unroll
        for (int k = 0; k < AV1MI_LR_WFIT_SUMS; k++) acc[k] = 0;
#pragma unroll 4
        for (int i = 0; i < 16; i++)
          if (active && ya + i < yb) {
            const int X = (int)g_win[i + 3][lane + 3], e = (int)src[(size_t)(ya + i) * stride + x] - X;
            int dv[3], dh[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
              const int o = 3 - k;
              dv[k] = (int)g_win[i + 3 - o][lane + 3] + (int)g_win[i + 3 + o][lane + 3] - 2 * X;
              dh[k] = (int)g_win[i + 3][lane + 3 - o] + (int)g_win[i + 3][lane + 3 + o] - 2 * X;
            }
            int n = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
              for (int k = j; k < 3; k++) { acc[AV1MI_WF_HVV + n] += dv[j] * dv[k]; acc[AV1MI_WF_HHH + n] += dh[j] * dh[k]; n++; }
#pragma unroll
            for (int j = 0; j < 3; j++) {
#pragma unroll
              for (int k = 0; k < 3; k++) acc[AV1MI_WF_HVH + j * 3 + k] += dv[j] * dh[k];
              acc[AV1MI_WF_CV + j] += dv[j] * e; acc[AV1MI_WF_CH + j] += dh[j] * e;
            }
          }
        unsigned long long *dst = (unsigned long long *)F.sums + (fit_base + ((lane >> 5) ? hi : lo)) * AV1MI_LR_WFIT_SUMS;
#pragma unroll
        for (int k = 0; k < AV1MI_LR_WFIT_SUMS; k++) {
          const unsigned long long v = half_sum64((unsigned long long)(long long)acc[k]);   // two's complement: the signed sum
          if ((lane & 31) == 0 && v) atomicAdd(&dst[k], v);
        }
      } else {
        wiener_h(bd, ya, yb, fh, lane);   // per-lane taps; g_mid is private to the lane's column
        if (mine)
          for (int y = ya; y < yb; y++) {
            const int v = wiener_v(y - ya, lane, fv, maxv);
            if constexpr (PHASE == 2) { const int d = v - (int)src[(size_t)y * stride + x]; sse += (unsigned long long)(d * d); }
            else out[(size_t)y * stride + x] = (PIX)v;
          }
      }
    }
    if constexpr (PHASE == 2) {
      const unsigned long long v = half_sum64(sse);
      if ((lane & 31) == 0 && v) atomicAdd(&F.err[fit_base + ((lane >> 5) ? hi : lo)], v);
    }
  }
}

// PHASE 4, in lr_pieces.h's coding-order walk.  A thread carries its plane's RefLrWiener, which starts every tile at Wiener_Taps_Mid in both
// passes and takes every Wiener unit's taps, fixed filters included.  With the self-guided fit its units' bits are written again as well:
// lr_fit_kernel.hip carried RefSgrXqd through units that have since become Wiener units, which the decoder's reference never sees.
__global__ void __launch_bounds__(64) lr_wfit_code_kernel(Av1miDevParams P, uint8_t *choice /* == B.choice */, BaseErr B, Av1miLrWfit F) {
  int ref[2][3];
  for (int p = 0; p < 2; p++) for (int j = 0; j < 3; j++) ref[p][j] = av1mi_wiener_tap_mid(j);
  int sref0 = -32, sref1 = 31;   // Sgrproj_Xqd_Mid
  lr_code_walk(P, [&](int pl, size_t u, size_t cu) {
    int8_t *r = F.rec + u * 8;
    int c = choice[cu];
    if (!r[1]) F.err[u] = ~0ull;
    else if (wfit_overrides(P, B, F, cu, u, pl > 0)) { c = AV1MI_LR_WFIT_CHOICE; choice[cu] = (uint8_t)c; }
    r[0] = (int8_t)c;
    if (B.fit_code && c >= 4 && c != AV1MI_LR_WFIT_CHOICE) {
      const int8_t *q = B.fit_rec + u * 4;
      const Av1miBitString g = av1mi_lr_sgr_code(q[1], q[2], q[3], sref0, sref1);
      B.fit_code[u * 2] = (uint32_t)g.bits; B.fit_code[u * 2 + 1] = (uint32_t)g.len;
      sref0 = q[2]; sref1 = q[3];
    }
    if (c != AV1MI_LR_WFIT_CHOICE && (c < 1 || c > 3)) return;
    int cv[3], ch[3];
    for (int j = 0; j < 3; j++) {
      if (c == AV1MI_LR_WFIT_CHOICE) { cv[j] = r[2 + j]; ch[j] = r[5 + j]; }
      else cv[j] = ch[j] = pl ? c_wiener_cand_uv[c - 1][j] : c_wiener_cand[c - 1][j];
    }
    const Av1miBitString b = av1mi_lr_wiener_code(pl > 0, cv, ch, ref);
    F.code[u * 3] = (uint32_t)b.bits; F.code[u * 3 + 1] = (uint32_t)(b.bits >> 32); F.code[u * 3 + 2] = (uint32_t)b.len;
    for (int j = pl > 0; j < 3; j++) { ref[0][j] = cv[j]; ref[1][j] = ch[j]; }
  });
}

}  // namespace

extern "C" hipError_t av1mi_launch_lr_wfit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                           const unsigned long long *unit_sse, const Av1miLrFit *sgr_fit, const Av1miLrWfit *wfit, int frame0,
                                           int count, hipStream_t stream) {
  const LrLaunch L = lr_launch_head(P, pre, cdef, src, out, frame0, count);
  choice += L.unit0;
  const Av1miLrFit G = sgr_fit ? sgr_fit->at_frame(frame0, L.fit_upf) : Av1miLrFit{};
  const BaseErr B = { choice, unit_sse + L.unit0 * 8, G.err, G.rec, G.code };
  const Av1miLrWfit F = wfit->at_frame(frame0, L.fit_upf);
  lr_launch_typed(L, [&](auto *a, auto *b, auto *s, auto *o) {
    using PIX = std::remove_pointer_t<decltype(o)>;
    hipLaunchKernelGGL((lr_wfit_kernel<PIX, 1>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, B, F);
    hipLaunchKernelGGL((lr_wfit_kernel<PIX, 2>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, B, F);
    hipLaunchKernelGGL((lr_wfit_kernel<PIX, 3>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, B, F);
  });
  hipLaunchKernelGGL(lr_wfit_code_kernel, dim3((L.code_threads + 63) / 64), dim3(64), 0, stream, L.R, choice, B, F);
  return hipGetLastError();
}
