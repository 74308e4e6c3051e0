// lr_fit_kernel.hip - the self-guided restoration fit (av1mi_params.enable_lr bit 8, AV1MI_LR_FIT): per
// restoration unit and parameter set the two weights by least squares (lr_fit_rule.h), the exact SSE of every fitted candidate, the
// decision over all 23 candidates, the winner applied, and the units' bit strings for symbolize.
//
// Replaces the self-guided parameter search of the SVT-AV1 worker behind `run_av1an`.  Normative part: §7.17.3 (box filter process
// and self guided filter process for any parameter set), §7.17.6 (stripes) and §5.11.58 (lr_sgr_set, the weights against RefSgrXqd).
//
// MI355X mapping: lr_kernel.hip's - one 64-lane wave per 16-row slice of a luma unit or of a pair of chroma units, lane = column, the
// same grid, window and grids in LDS (17 KB per wave + a 128-byte table of the units' weights).  Four launches after lr_kernel.hip's
// phase 0 (the SSE of the seven fixed candidates):
//   1 sums    per set the A / B grids with the set's strengths, the five sums per lane, reduced per unit, one 64-bit atomic per sum
//             (14-bit terms; a unit of 256 luma samples has at most 383 x 391 of them: |sum| < 2^46)
//   2 SSE     every slice solves its units' weights from the complete sums (32 lanes, one (unit, set) each), filters again and adds
//             its exact SSE per set
//   3 decide  first minimum over the 23 candidates - of the error or, with the rate term (lr_rate_rule.h), of J, the fitted weights' bits
//             counted beside the solve - the unit's record, and the winner of any kind applied (with the padding and,
//             without chroma restoration, the chroma copy of lr_kernel.hip's phase 1)
//   4 codes   one thread per (frame, plane, tile) carries RefSgrXqd over the tile's units in coding order
// Sets 11, 12, 13 share their r = 1 strengths with sets 2, 5, 8: the sets run in an order that puts them behind those, and a pass whose
// grid is already in LDS is not computed again.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "lr_fit_rule.h"
#include "lr_rate_rule.h"

namespace {

#include "lr_pieces.h"

// [unit of the wave's section][set]: -1 absent, else (xqd0 + 128) | (xqd1 + 128) << 8 and, for a decision with the rate term, Lc << 16
__shared__ int g_fitw[2][AV1MI_LR_FIT_SETS];

// the sets in the order 0 1 2 11 3 4 5 12 6 7 8 13 9 10 14 15, a nibble each
__device__ __forceinline__ int fit_order(int i) { return (int)((0xFEA9D876C543B210ull >> (4 * i)) & 15); }

// the grids of set t in LDS; e1_in_lds: the strength the r = 1 grid was last computed with for this window (-1: none)
__device__ __forceinline__ void fit_grids(int bd, int ya, int yb, int lane, int t, int &e1_in_lds) {
  __syncthreads();   // the readers of the previous grids are done
  if (av1mi_sgr_r0(t)) box_grid<0>(bd, ya, yb, lane, av1mi_sgr_eps0(t));
  if (av1mi_sgr_r1(t) && av1mi_sgr_eps1(t) != e1_in_lds) { e1_in_lds = av1mi_sgr_eps1(t); box_grid<1>(bd, ya, yb, lane, e1_in_lds); }
  __syncthreads();
}

// PHASE 1: sums; 2: solve and SSE; 3: decide and apply.  The grid is lr_unit_kernel's, the wave's place in it lr_pieces.h's lr_wave.  Fit
// buffers are [frame][plane 0..2][unit], the fixed candidates' choice and unit_sse [frame][plane][unit] over the restored planes.
template <typename PIX, int PHASE>
__global__ void __launch_bounds__(64) lr_fit_kernel(Av1miDevParams P, const PIX *__restrict__ pre, const PIX *__restrict__ cdef,
                                                   const PIX *__restrict__ src, PIX *__restrict__ out, uint8_t *__restrict__ choice,
                                                   const unsigned long long *__restrict__ unit_sse, Av1miLrFit F) {
  // the blocks are those of the cells (the units of lr_unit_shift 0); sums, weights, errors and records are those of the unit a cell lies in
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
    if constexpr (PHASE >= 2) {
      // the weights of both units and every set from the complete sums
      __syncthreads();
      if (lane < 32) {
        const int h = lane >> 4, t = lane & 15;
        int w0 = 0, w1 = 0, ok = 0;
        if ((F.mask >> t) & 1) ok = av1mi_lr_fit_solve(t, F.sums + ((fit_base + (h ? hi : lo)) * AV1MI_LR_FIT_SETS + t) * 5, &w0, &w1);
        int lc = 0;
        if constexpr (PHASE == 3) { if (ok && P.lr_lambda) lc = av1mi_lr_sgr_lc(t, w0, w1); }
        g_fitw[h][t] = ok ? ((w0 + 128) | ((w1 + 128) << 8) | (lc << 16)) : -1;
      }
      __syncthreads();
    }
    [[maybe_unused]] int best[2] = { 0, 0 }, bset[2] = { 0, 0 }, bw0[2] = { 0, 0 }, bw1[2] = { 0, 0 };
    if constexpr (PHASE == 3) {
      const LrRate rate = lr_rate(P, sub);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const unsigned long long *e = F.err + (fit_base + (h ? hi : lo)) * AV1MI_LR_FIT_CANDS;
        unsigned long long bj;
        best[h] = lr_decide(unit_sse + (sse_base + (h ? hi : lo)) * 8, 6, rate, bj);   // ... and on over the fitted sets
        for (int t = 0; t < AV1MI_LR_FIT_SETS; t++) {
          if (g_fitw[h][t] < 0) continue;
          const unsigned long long j = av1mi_lr_j(e[7 + t], rate.lambda, av1mi_lr_b16(g_fitw[h][t] >> 16, rate.t16_sgr));
          if (j < bj) { bj = j; best[h] = 7 + t; }
        }
        if (best[h] >= 7) { const int fw = g_fitw[h][best[h] - 7]; bset[h] = best[h] - 7; bw0[h] = (fw & 255) - 128; bw1[h] = ((fw >> 8) & 255) - 128; }
        else if (best[h] >= 4) { bset[h] = c_sgr_cand[best[h] - 4][0]; bw0[h] = c_sgr_cand[best[h] - 4][1]; bw1[h] = c_sgr_cand[best[h] - 4][2]; }
      }
      if (lr_records(P, w, unit, x, active)) {   // the unit's record
        const unsigned long long *usse = unit_sse + (sse_base + unit) * 8;
        unsigned long long *e = F.err + (fit_base + unit) * AV1MI_LR_FIT_CANDS;
        for (int k = 0; k < 7; k++) e[k] = usse[k];
        for (int t = 0; t < AV1MI_LR_FIT_SETS; t++) if (g_fitw[hsel][t] < 0) e[7 + t] = ~0ull;   // absent (no slice reads these)
        int8_t *r = F.rec + (fit_base + unit) * 4;
        r[0] = (int8_t)best[hsel]; r[1] = (int8_t)bset[hsel]; r[2] = (int8_t)bw0[hsel]; r[3] = (int8_t)bw1[hsel];
        choice[sse_base + unit] = (uint8_t)best[hsel];
      }
    }
    for (int st = lr_first_stripe(y0, sub); lr_stripe_row0(st, sub) < y1; st++) {
      const LrStripe S = lr_stripe(st, y0, y1, sub);
      const int ya = S.ya, yb = S.yb;
      if constexpr (PHASE <= 2) {
        __syncthreads();
        lr_stage<PIX>(cdef, pre, xs, ya, yb, S.s0, S.s1, w.W, w.H, stride, lane);
        __syncthreads();
        int cur[16], sv[16];
        lr_load_cur_src<PIX>(src, stride, x, active, ya, yb, lane, cur, sv);
        int e1_in_lds = -1;
#pragma nounroll
        for (int oi = 0; oi < AV1MI_LR_FIT_SETS; oi++) {
          const int t = fit_order(oi), r0 = av1mi_sgr_r0(t), r1 = av1mi_sgr_r1(t);
          if constexpr (PHASE == 1) { if (!((F.mask >> t) & 1)) continue; }
          else { if (g_fitw[0][t] < 0 && g_fitw[1][t] < 0) continue; }
          fit_grids(bd, ya, yb, lane, t, e1_in_lds);
          if constexpr (PHASE == 1) {
            long long acc[5] = { 0, 0, 0, 0, 0 };
#pragma unroll
            for (int i = 0; i < 16; i++)
              if (active && ya + i < yb) {
                const int uu = cur[i] << 4, s = (sv[i] << 4) - uu;
                const int f0 = r0 ? box_flt0(lane, ya + i, ya, cur[i]) - uu : 0, f1 = r1 ? box_flt1(lane, ya + i, ya, cur[i]) - uu : 0;
                acc[0] += (long long)f0 * f0; acc[1] += (long long)f0 * f1; acc[2] += (long long)f1 * f1;
                acc[3] += (long long)f0 * s; acc[4] += (long long)f1 * s;
              }
            unsigned long long *dst = (unsigned long long *)F.sums + ((fit_base + ((lane >> 5) ? hi : lo)) * AV1MI_LR_FIT_SETS + t) * 5;
#pragma unroll
            for (int k = 0; k < 5; k++) {
              const unsigned long long v = half_sum64((unsigned long long)acc[k]);   // two's complement: the signed sum
              if ((lane & 31) == 0 && v) atomicAdd(&dst[k], v);
            }
          } else {
            const int fw = g_fitw[hsel][t], w0 = (fw & 255) - 128, w1 = ((fw >> 8) & 255) - 128;   // (PHASE 2: no Lc above)
            unsigned long long sse = 0;
#pragma unroll
            for (int i = 0; i < 16; i++)
              if (active && fw >= 0 && ya + i < yb) {
                const int fl0 = r0 ? box_flt0(lane, ya + i, ya, cur[i]) : 0, fl1 = r1 ? box_flt1(lane, ya + i, ya, cur[i]) : 0;
                const int d = box_blend(cur[i], r0, r1, fl0, fl1, w0, w1, maxv) - sv[i];
                sse += (unsigned long long)(d * d);
              }
            const unsigned long long v = half_sum64(sse);
            if ((lane & 31) == 0 && v) atomicAdd(&F.err[(fit_base + ((lane >> 5) ? hi : lo)) * AV1MI_LR_FIT_CANDS + 7 + t], v);
          }
        }
      } else {
        const int nh = lo != hi ? 2 : 1;
        if (best[0] || (nh == 2 && best[1])) {
          __syncthreads();
          lr_stage<PIX>(cdef, pre, xs, ya, yb, S.s0, S.s1, w.W, w.H, stride, lane);
          __syncthreads();
        }
        int e1_in_lds = -1;
#pragma unroll
        for (int h = 0; h < 2; h++) {
          if (h >= nh) break;
          const int b = best[h];
          const bool mine = active && (nh == 1 || (lane >> 5) == h);
          if (b == 0) {
            if (mine) for (int y = ya; y < yb; y++) out[(size_t)y * stride + x] = cdef[(size_t)y * stride + x];
          } else if (b <= 3) {
            int tf[7];
            if (sub) taps_of_uv(b - 1, tf); else taps_of(b - 1, tf);
            wiener_h(bd, ya, yb, tf, lane);   // g_mid is private to the lane's column
            if (mine) for (int y = ya; y < yb; y++) out[(size_t)y * stride + x] = (PIX)wiener_v(y - ya, lane, tf, maxv);
          } else {
            const int t = bset[h], r0 = av1mi_sgr_r0(t), r1 = av1mi_sgr_r1(t);
            fit_grids(bd, ya, yb, lane, t, e1_in_lds);
            if (mine)
              for (int y = ya; y < yb; y++) {
                const int c = (int)g_win[y - ya + 3][lane + 3];
                const int fl0 = r0 ? box_flt0(lane, y, ya, c) : 0, fl1 = r1 ? box_flt1(lane, y, ya, c) : 0;
                out[(size_t)y * stride + x] = (PIX)box_blend(c, r0, r1, fl0, fl1, bw0[h], bw1[h], maxv);
              }
          }
        }
      }
    }
  }
  // (without chroma restoration there are luma waves only: they copy the co-located chroma)
  if constexpr (PHASE == 3) lr_tail<PIX>(P, cdef, out, sub, !P.lr_chroma, w.last_row, w.last_col, w.x0, x1, y0, y1, stride, lane);
}

// PHASE 4: the bit strings of the self-guided units, fixed candidates included, in lr_pieces.h's coding-order walk.  A thread carries its
// plane's RefSgrXqd, which starts every tile at Sgrproj_Xqd_Mid and takes every self-guided unit's weights, implied ones included.
__global__ void __launch_bounds__(64) lr_fit_code_kernel(Av1miDevParams P, Av1miLrFit F) {
  int ref0 = -32, ref1 = 31;
  lr_code_walk(P, [&](int, size_t u, size_t) {
    const int8_t *r = F.rec + u * 4;
    if (r[0] < 4) return;
    const Av1miBitString b = av1mi_lr_sgr_code(r[1], r[2], r[3], ref0, ref1);
    F.code[u * 2] = (uint32_t)b.bits; F.code[u * 2 + 1] = (uint32_t)b.len;
    ref0 = r[2]; ref1 = r[3];
  });
}

}  // namespace

extern "C" hipError_t av1mi_launch_lr_fit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                          const unsigned long long *unit_sse, const Av1miLrFit *fit, int frame0, int count, hipStream_t stream) {
  const LrLaunch L = lr_launch_head(P, pre, cdef, src, out, frame0, count);
  choice += L.unit0; unit_sse += L.unit0 * 8;
  const Av1miLrFit F = fit->at_frame(frame0, L.fit_upf);
  lr_launch_typed(L, [&](auto *a, auto *b, auto *s, auto *o) {
    using PIX = std::remove_pointer_t<decltype(o)>;
    hipLaunchKernelGGL((lr_fit_kernel<PIX, 1>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, choice, unit_sse, F);
    hipLaunchKernelGGL((lr_fit_kernel<PIX, 2>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, choice, unit_sse, F);
    hipLaunchKernelGGL((lr_fit_kernel<PIX, 3>), dim3(L.grid), dim3(64), 0, stream, L.R, a, b, s, o, choice, unit_sse, F);
  });
  hipLaunchKernelGGL(lr_fit_code_kernel, dim3((L.code_threads + 63) / 64), dim3(64), 0, stream, L.R, F);
  return hipGetLastError();
}
