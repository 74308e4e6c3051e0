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
//   3 override  a unit whose fitted error is strictly below its winner's is filtered again with the fitted taps (read-only on every
//               table: the slices of a unit take the same decision)
//   4 codes     one thread per (frame, plane, tile) walks the tile's units in coding order: the final choice (23 = fitted) into the
//               record and the choice table, and the bits of every Wiener unit against the carried RefLrWiener
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "wiener_fit_rule.h"

namespace {

#include "lr_pieces.h"

__shared__ int g_wtap[2][8];   // [unit of the wave's section]: present, cv0 .. cv2, ch0 .. ch2

__device__ __forceinline__ void taps7(const int *c, int *f) {
  f[0] = f[6] = c[0]; f[1] = f[5] = c[1]; f[2] = f[4] = c[2]; f[3] = 128 - 2 * (c[0] + c[1] + c[2]);
}

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

// PHASE 1: sums; 2: solve and SSE; 3: override.  The grid is lr_unit_kernel's.
template <typename PIX, int PHASE>
__global__ void __launch_bounds__(64) lr_wfit_kernel(Av1miDevParams P, const PIX *__restrict__ pre, const PIX *__restrict__ cdef,
                                                    const PIX *__restrict__ src, PIX *__restrict__ out, BaseErr B, Av1miLrWfit F) {
  // the blocks are those of the cells (the units of lr_unit_shift 0); sums, taps, errors and records are those of the unit a cell lies in
  const int crows = av1mi_lr_cell_rows(P), ccols = av1mi_lr_cell_cols(P), cells = crows * ccols;
  const int ush = P.lr_unit_shift, urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int lane = threadIdx.x;
  const int luma_blocks = P.n_frames * cells * LR_SLICES;
  int f, pl, cr, slice, x0, x1, ccl;
  if ((int)blockIdx.x < luma_blocks) {
    const int item = blockIdx.x / LR_SLICES, cell = item % cells;
    slice = blockIdx.x % LR_SLICES; f = item / cells; pl = 0; cr = cell / ccols; ccl = cell % ccols;
    x0 = ccl * 64; x1 = ccl == ccols - 1 ? P.true_w : x0 + 64;
  } else {
    if (!P.lr_chroma) return;
    const int item = (int)blockIdx.x - luma_blocks, pairs = (ccols + 1) >> 1, rest = item / LR_SLICES_C;
    const int pc = rest % pairs;
    slice = item % LR_SLICES_C; cr = rest / pairs % crows; pl = 1 + rest / (pairs * crows) % 2; f = rest / (pairs * crows * 2); ccl = -1;
    if (f >= P.n_frames) return;
    x0 = pc * 64; x1 = pc == pairs - 1 ? (P.true_w + 1) >> 1 : x0 + 64;
  }
  const int ur = av1mi_lr_unit_of_cell(cr, urows, ush);
  const int sub = pl > 0;
  const int W = sub ? (P.true_w + 1) >> 1 : P.true_w, H = sub ? (P.true_h + 1) >> 1 : P.true_h, stride = sub ? P.stride_c : P.stride_y;
  const int sh = 64 >> sub, so = 8 >> sub;   // stripe height = cell size, and the row offset of both
  const size_t fo = (size_t)f * P.frame_samples + (pl == 0 ? 0 : (pl == 1 ? P.plane_off_u : P.plane_off_v));
  pre += fo; cdef += fo; src += fo; out += fo;
  const int uy0 = av1mi_lr_row0(cr, 0, sub), uy1 = av1mi_lr_row1(cr, crows, 0, sub, H);   // the cell row's rows
  const int y0 = uy0 + slice * 16, y1 = y0 + 16 < uy1 ? y0 + 16 : uy1;
  if (y0 >= uy1) return;
  const int maxv = (1 << P.bit_depth) - 1, bd = P.bit_depth;
  const size_t sse_base = ((size_t)f * (P.lr_chroma ? 3 : 1) + pl) * per + (size_t)ur * ucols;   // unit (ur, 0) of the plane
  const size_t fit_base = ((size_t)f * 3 + pl) * per + (size_t)ur * ucols;
  for (int xs = x0; xs < x1; xs += 64) {
    const int x = xs + lane;
    const bool active = x < x1;
    // the section's units: lanes 0-31 are in `lo`, lanes 32-63 in `hi` (one unit: luma, a last chroma cell on its own, and two chroma
    // cells of one larger unit)
    const int lo = av1mi_lr_unit_of_cell(ccl >= 0 ? ccl : min(ccols - 1, xs >> 5), ucols, ush);
    const int hi = av1mi_lr_unit_of_cell(ccl >= 0 ? ccl : min(ccols - 1, (xs >> 5) + 1), ucols, ush);
    const int hsel = lo != hi ? lane >> 5 : 0, unit = hsel ? hi : lo;
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
      taps7(&g_wtap[hsel][1], fv); taps7(&g_wtap[hsel][4], fh);
      // the unit's record (present, taps), by the lane of its first column in the first slice of the unit's first cell; the choice
      // follows in phase 4
      if (slice == 0 && cr == av1mi_lr_first_cell(ur, ush) && active && x == av1mi_lr_first_cell(unit, ush) * sh) {
        int8_t *r = F.rec + (fit_base + unit) * 8;
        for (int j = 0; j < 7; j++) r[1 + j] = (int8_t)g_wtap[hsel][j];
      }
    }
    if constexpr (PHASE == 3) {
      // both units' decisions in every lane: the stripe loop below stays uniform
      bool ov[2];
      for (int h = 0; h < 2; h++) {
        const size_t u = fit_base + (h ? hi : lo);
        ov[h] = F.rec[u * 8 + 1] != 0 && F.err[u] < base_err_of(B, sse_base + (h ? hi : lo), u);
      }
      const int8_t *r = F.rec + (fit_base + unit) * 8;
      int cv[3] = { r[2], r[3], r[4] }, ch[3] = { r[5], r[6], r[7] };
      taps7(cv, fv); taps7(ch, fh);
      mine = active && ov[hsel];
      any = ov[0] || ov[1];
    }
    if (!any) continue;
    [[maybe_unused]] unsigned long long sse = 0;
    for (int st = (y0 + so) / sh; st * sh - so < y1; st++) {
      const int s0 = st * sh - so, s1 = s0 + sh - 1;
      const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;   // <= 16 rows
      __syncthreads();
      lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, W, H, stride, lane);
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

// PHASE 4.  One thread per (frame, restored plane, tile) walks the tile's units in coding order - unit (r, c) of every plane is read
// with superblock (r << lr_unit_shift, c << lr_unit_shift), so a tile may start no unit - and carries the plane's RefLrWiener, which starts every tile at Wiener_Taps_Mid in both passes and takes
// every Wiener unit's taps, fixed filters included.  With the self-guided fit its units' bits are written again as well: lr_fit_kernel.hip
// carried RefSgrXqd through units that have since become Wiener units, which the decoder's reference never sees.
__global__ void __launch_bounds__(64) lr_wfit_code_kernel(Av1miDevParams P, uint8_t *choice /* == B.choice */, BaseErr B, Av1miLrWfit F) {
  const int urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int nplanes = P.lr_chroma ? 3 : 1, tiles = P.tile_rows * P.tile_cols;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= P.n_frames * nplanes * tiles) return;
  const int tile = idx % tiles, pl = idx / tiles % nplanes, f = idx / (tiles * nplanes);
  const int tr = tile / P.tile_cols, tc = tile % P.tile_cols, tsb = P.tile_sb;
  int ref[2][3];
  for (int p = 0; p < 2; p++) for (int j = 0; j < 3; j++) ref[p][j] = av1mi_wiener_tap_mid(j);
  int sref0 = -32, sref1 = 31;   // Sgrproj_Xqd_Mid
  for (int si = 0; si < tsb * tsb; si++) {
    const int sbr = tr * tsb + si / tsb, sbc = tc * tsb + si % tsb;
    const int ur = av1mi_lr_sb_unit(sbr, urows, P.lr_unit_shift), uc = av1mi_lr_sb_unit(sbc, ucols, P.lr_unit_shift);
    if (sbr >= P.sb_rows || sbc >= P.sb_cols || ur < 0 || uc < 0) continue;
    const size_t u = ((size_t)f * 3 + pl) * per + (size_t)ur * ucols + uc, cu = ((size_t)f * nplanes + pl) * per + (size_t)ur * ucols + uc;
    int8_t *r = F.rec + u * 8;
    int c = choice[cu];
    if (!r[1]) F.err[u] = ~0ull;
    else if (F.err[u] < base_err_of(B, cu, u)) { c = AV1MI_LR_WFIT_CHOICE; choice[cu] = (uint8_t)c; }
    r[0] = (int8_t)c;
    if (B.fit_code && c >= 4 && c != AV1MI_LR_WFIT_CHOICE) {
      const int8_t *q = B.fit_rec + u * 4;
      const Av1miBitString g = av1mi_lr_sgr_code(q[1], q[2], q[3], sref0, sref1);
      B.fit_code[u * 2] = (uint32_t)g.bits; B.fit_code[u * 2 + 1] = (uint32_t)g.len;
      sref0 = q[2]; sref1 = q[3];
    }
    if (c != AV1MI_LR_WFIT_CHOICE && (c < 1 || c > 3)) continue;
    int cv[3], ch[3];
    for (int j = 0; j < 3; j++) {
      if (c == AV1MI_LR_WFIT_CHOICE) { cv[j] = r[2 + j]; ch[j] = r[5 + j]; }
      else cv[j] = ch[j] = pl ? c_wiener_cand_uv[c - 1][j] : c_wiener_cand[c - 1][j];
    }
    const Av1miBitString b = av1mi_lr_wiener_code(pl > 0, cv, ch, ref);
    F.code[u * 3] = (uint32_t)b.bits; F.code[u * 3 + 1] = (uint32_t)(b.bits >> 32); F.code[u * 3 + 2] = (uint32_t)b.len;
    for (int j = pl > 0; j < 3; j++) { ref[0][j] = cv[j]; ref[1][j] = ch[j]; }
  }
}

template <typename PIX>
void launch_wfit_typed(const Av1miDevParams &R, int grid, const void *pre, const void *cdef, const void *src, void *out, const BaseErr &B,
                       const Av1miLrWfit &F, hipStream_t stream) {
  const PIX *a = (const PIX *)pre, *b = (const PIX *)cdef, *s = (const PIX *)src;
  PIX *o = (PIX *)out;
  hipLaunchKernelGGL((lr_wfit_kernel<PIX, 1>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, B, F);
  hipLaunchKernelGGL((lr_wfit_kernel<PIX, 2>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, B, F);
  hipLaunchKernelGGL((lr_wfit_kernel<PIX, 3>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, B, F);
}

}  // namespace

extern "C" hipError_t av1mi_launch_lr_wfit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                           const unsigned long long *unit_sse, const Av1miLrFit *sgr_fit, const Av1miLrWfit *wfit, int frame0,
                                           int count, hipStream_t stream) {
  const Av1miDevParams R = av1mi_frame_range(*P, frame0, count);
  const size_t upf = (size_t)av1mi_lr_frame_units(R), fit_upf = (size_t)3 * av1mi_lr_unit_rows(R) * av1mi_lr_unit_cols(R);
  pre = av1mi_frame_at(R, pre, frame0); cdef = av1mi_frame_at(R, cdef, frame0); src = av1mi_frame_at(R, src, frame0); out = av1mi_frame_at(R, out, frame0);
  choice += frame0 * upf;
  BaseErr B;
  B.choice = choice; B.unit_sse = unit_sse + frame0 * upf * 8;
  B.fit_err = sgr_fit ? sgr_fit->err + frame0 * fit_upf * AV1MI_LR_FIT_CANDS : nullptr;
  B.fit_rec = sgr_fit ? sgr_fit->rec + frame0 * fit_upf * 4 : nullptr;
  B.fit_code = sgr_fit ? sgr_fit->code + frame0 * fit_upf * 2 : nullptr;
  Av1miLrWfit F = *wfit;
  F.err += frame0 * fit_upf; F.rec += frame0 * fit_upf * 8; F.sums += frame0 * fit_upf * AV1MI_LR_WFIT_SUMS; F.code += frame0 * fit_upf * 3;
  const int grid = av1mi_lr_grid(R, count);   // == av1mi_launch_lr's
  if (R.bit_depth == 8) launch_wfit_typed<uint8_t>(R, grid, pre, cdef, src, out, B, F, stream);
  else launch_wfit_typed<uint16_t>(R, grid, pre, cdef, src, out, B, F, stream);
  const int threads = count * (R.lr_chroma ? 3 : 1) * R.tile_rows * R.tile_cols;
  hipLaunchKernelGGL(lr_wfit_code_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, R, choice, B, F);
  return hipGetLastError();
}
