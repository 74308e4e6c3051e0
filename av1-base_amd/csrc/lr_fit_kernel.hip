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
//   3 decide  first minimum over the 23 candidates, the unit's record, and the winner of any kind applied (with the padding and,
//             without chroma restoration, the chroma copy of lr_kernel.hip's phase 1)
//   4 codes   one thread per (frame, plane, tile) carries RefSgrXqd over the tile's units in coding order
// Sets 11, 12, 13 share their r = 1 strengths with sets 2, 5, 8: the sets run in an order that puts them behind those, and a pass whose
// grid is already in LDS is not computed again.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "lr_fit_rule.h"

namespace {

#include "lr_pieces.h"

__shared__ int g_fitw[2][AV1MI_LR_FIT_SETS];   // [unit of the wave's section][set]: -1 absent, else (xqd0 + 128) | (xqd1 + 128) << 8

// the sets in the order 0 1 2 11 3 4 5 12 6 7 8 13 9 10 14 15, a nibble each
__device__ __forceinline__ int fit_order(int i) { return (int)((0xFEA9D876C543B210ull >> (4 * i)) & 15); }

// fit_ab and fit_grid are lr_kernel.hip's sgr_ab and sgr_grid with the strength as an argument (those stay as they are, with the
// strengths of set 9 as constants): the two pairs must change together - arithmetic, window rows, grid layout.
// A and B from the box sums of a window of n samples with the strength's scale s = Round(2^20 / (n^2 eps))
__device__ __forceinline__ void fit_ab(uint32_t a, uint32_t b, int bd, uint32_t n, uint32_t s, uint32_t one_by_n, uint32_t &A, int32_t &B) {
  const uint32_t a8 = (a + ((1u << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8));
  const uint32_t d = (b + ((1u << (bd - 8)) >> 1)) >> (bd - 8);
  const uint32_t p = a8 * n > d * d ? a8 * n - d * d : 0;
  const uint32_t z = (uint32_t)(((unsigned long long)p * s + (1u << 19)) >> 20);
  const uint32_t a2 = z >= 255 ? 256 : (z == 0 ? 1 : ((z << 8) + z / 2) / (z + 1));
  A = a2;
  B = (int32_t)(((unsigned long long)(256 - a2) * b * one_by_n + (1u << 11)) >> 12);
}

// lr_kernel.hip's sgr_grid with the strength as an argument: A/B of pass PASS for the section rows ya - 1 .. yb (<= 18 rows; pass 0 on
// odd rows only, <= 9) and columns xs - 1 .. xs + 64 from the staged window (rows ya - 3 .. yb + 2)
template <int PASS>
__device__ __forceinline__ void fit_grid(int bd, int ya, int yb, int lane, int eps) {
  constexpr int R = PASS == 0 ? 2 : 1, WN = 2 * R + 1;
  constexpr uint32_t n = WN * WN, one_by_n = ((1u << 12) + n / 2) / n;
  const uint32_t n2e = n * n * (uint32_t)eps, s = ((1u << 20) + n2e / 2) / n2e;
  const uint16_t (*win)[72] = g_win;
  uint32_t h1[WN], h2[WN];
#pragma unroll
  for (int t = 0; t < WN; t++) { h1[t] = 0; h2[t] = 0; }
  for (int yy = ya - 1 - R; yy <= yb + R; yy++) {
    const uint16_t *row = win[yy - (ya - 3)] + lane + 3 - R;
    uint32_t r1 = 0, r2 = 0;
#pragma unroll
    for (int t = 0; t < WN; t++) { const uint32_t c = row[t]; r1 += c; r2 += c * c; }
#pragma unroll
    for (int t = 0; t < WN - 1; t++) { h1[t] = h1[t + 1]; h2[t] = h2[t + 1]; }
    h1[WN - 1] = r1; h2[WN - 1] = r2;
    const int yc = yy - R;
    if (yc >= ya - 1 && (PASS == 1 || (yc & 1))) {
      uint32_t b = 0, a = 0;
#pragma unroll
      for (int t = 0; t < WN; t++) { b += h1[t]; a += h2[t]; }
      uint32_t A; int32_t B;
      fit_ab(a, b, bd, n, s, one_by_n, A, B);
      if (PASS == 0) { g_sgrA0[(yc - (ya - 1)) >> 1][lane + 1] = (uint16_t)A; g_sgrB0[(yc - (ya - 1)) >> 1][lane + 1] = B; }
      else { g_sgrA1[yc - (ya - 1)][lane + 1] = (uint16_t)A; g_sgrB1[yc - (ya - 1)][lane + 1] = B; }
    }
  }
  const int rows = yb - ya + 2;
  for (int task = lane; task < rows * 2; task += 64) {
    const int ri = task >> 1, side = task & 1;
    const int yc = ya - 1 + ri, j = side ? 67 : 2;
    if (PASS == 0 && !(yc & 1)) continue;
    uint32_t a = 0, b = 0;
    for (int dy = -R; dy <= R; dy++) {
      const uint16_t *row = win[yc + dy - (ya - 3)] + j - R;
#pragma unroll
      for (int t = 0; t < WN; t++) { const uint32_t c = row[t]; b += c; a += c * c; }
    }
    uint32_t A; int32_t B;
    fit_ab(a, b, bd, n, s, one_by_n, A, B);
    if (PASS == 0) { g_sgrA0[ri >> 1][side ? 65 : 0] = (uint16_t)A; g_sgrB0[ri >> 1][side ? 65 : 0] = B; }
    else { g_sgrA1[ri][side ? 65 : 0] = (uint16_t)A; g_sgrB1[ri][side ? 65 : 0] = B; }
  }
}

// box-filter output of the r = 1 pass / the r = 2 pass for sample (xs + lane, y); cur = the CDEF sample
__device__ __forceinline__ int fit_flt1(int lane, int y, int ya, int cur) {
  const int ri = y - (ya - 1), c = lane + 1;
  int a = 0, b = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int w = (dx == 0 || dy == 0) ? 4 : 3;
      a += w * (int)g_sgrA1[ri + dy][c + dx]; b += w * g_sgrB1[ri + dy][c + dx];
    }
  return (a * cur + b + (1 << 8)) >> 9;
}
__device__ __forceinline__ int fit_flt0(int lane, int y, int ya, int cur) {
  const int ri = y - (ya - 1), c = lane + 1;
  int a = 0, b = 0;
  if (y & 1) {
    const int r0 = ri >> 1;
    a = 5 * (int)g_sgrA0[r0][c - 1] + 6 * (int)g_sgrA0[r0][c] + 5 * (int)g_sgrA0[r0][c + 1];
    b = 5 * g_sgrB0[r0][c - 1] + 6 * g_sgrB0[r0][c] + 5 * g_sgrB0[r0][c + 1];
    return (a * cur + b + (1 << 7)) >> 8;
  }
#pragma unroll
  for (int dy = -1; dy <= 1; dy += 2) {
    const int r0 = (ri + dy) >> 1;
    a += 5 * (int)g_sgrA0[r0][c - 1] + 6 * (int)g_sgrA0[r0][c] + 5 * (int)g_sgrA0[r0][c + 1];
    b += 5 * g_sgrB0[r0][c - 1] + 6 * g_sgrB0[r0][c] + 5 * g_sgrB0[r0][c + 1];
  }
  return (a * cur + b + (1 << 8)) >> 9;
}
// §7.17.3's blend; a pass whose radius is zero contributes u
__device__ __forceinline__ int fit_blend(int cur, int r0, int r1, int flt0, int flt1, int w0, int w1, int maxv) {
  const int u = cur << 4, w2 = 128 - w0 - w1;
  const int v = w1 * u + w0 * (r0 ? flt0 : u) + w2 * (r1 ? flt1 : u);
  return clampi((v + (1 << 10)) >> 11, 0, maxv);
}

// the grids of set t in LDS; e1_in_lds: the strength the r = 1 grid was last computed with for this window (-1: none)
__device__ __forceinline__ void fit_grids(int bd, int ya, int yb, int lane, int t, int &e1_in_lds) {
  __syncthreads();   // the readers of the previous grids are done
  if (av1mi_sgr_r0(t)) fit_grid<0>(bd, ya, yb, lane, av1mi_sgr_eps0(t));
  if (av1mi_sgr_r1(t) && av1mi_sgr_eps1(t) != e1_in_lds) { e1_in_lds = av1mi_sgr_eps1(t); fit_grid<1>(bd, ya, yb, lane, e1_in_lds); }
  __syncthreads();
}

// PHASE 1: sums; 2: solve and SSE; 3: decide and apply.  The grid is lr_unit_kernel's: luma blocks (unit x LR_SLICES), then with chroma
// restoration per frame and plane unit rows x pairs of unit columns x LR_SLICES_C.  Fit buffers are [frame][plane 0..2][unit], the fixed
// candidates' choice and unit_sse [frame][plane][unit] over the restored planes.
template <typename PIX, int PHASE>
__global__ void __launch_bounds__(64) lr_fit_kernel(Av1miDevParams P, const PIX *__restrict__ pre, const PIX *__restrict__ cdef,
                                                   const PIX *__restrict__ src, PIX *__restrict__ out, uint8_t *__restrict__ choice,
                                                   const unsigned long long *__restrict__ unit_sse, Av1miLrFit F) {
  // the blocks are those of the cells (the units of lr_unit_shift 0); sums, weights, errors and records are those of the unit a cell lies in
  const int crows = av1mi_lr_cell_rows(P), ccols = av1mi_lr_cell_cols(P), cells = crows * ccols;
  const int ush = P.lr_unit_shift, urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int lane = threadIdx.x;
  const int luma_blocks = P.n_frames * cells * LR_SLICES;
  int f, pl, cr, slice, x0, x1, ccl, last_col;
  if ((int)blockIdx.x < luma_blocks) {
    const int item = blockIdx.x / LR_SLICES, cell = item % cells;
    slice = blockIdx.x % LR_SLICES; f = item / cells; pl = 0; cr = cell / ccols; ccl = cell % ccols;
    x0 = ccl * 64; last_col = ccl == ccols - 1; x1 = last_col ? P.true_w : x0 + 64;
  } else {
    if (!P.lr_chroma) return;
    const int item = (int)blockIdx.x - luma_blocks, pairs = (ccols + 1) >> 1, rest = item / LR_SLICES_C;
    const int pc = rest % pairs;
    slice = item % LR_SLICES_C; cr = rest / pairs % crows; pl = 1 + rest / (pairs * crows) % 2; f = rest / (pairs * crows * 2); ccl = -1;
    if (f >= P.n_frames) return;
    x0 = pc * 64; last_col = pc == pairs - 1; x1 = last_col ? (P.true_w + 1) >> 1 : x0 + 64;
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
    if constexpr (PHASE >= 2) {
      // the weights of both units and every set from the complete sums
      __syncthreads();
      if (lane < 32) {
        const int h = lane >> 4, t = lane & 15;
        int w0 = 0, w1 = 0, ok = 0;
        if ((F.mask >> t) & 1) ok = av1mi_lr_fit_solve(t, F.sums + ((fit_base + (h ? hi : lo)) * AV1MI_LR_FIT_SETS + t) * 5, &w0, &w1);
        g_fitw[h][t] = ok ? ((w0 + 128) | ((w1 + 128) << 8)) : -1;
      }
      __syncthreads();
    }
    [[maybe_unused]] int best[2] = { 0, 0 }, bset[2] = { 0, 0 }, bw0[2] = { 0, 0 }, bw1[2] = { 0, 0 };
    if constexpr (PHASE == 3) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const unsigned long long *usse = unit_sse + (sse_base + (h ? hi : lo)) * 8, *e = F.err + (fit_base + (h ? hi : lo)) * AV1MI_LR_FIT_CANDS;
        unsigned long long bs = usse[0];
        for (int k = 1; k < 7; k++) { const unsigned long long s = usse[k]; if (s < bs) { bs = s; best[h] = k; } }
        for (int t = 0; t < AV1MI_LR_FIT_SETS; t++) {
          if (g_fitw[h][t] < 0) continue;
          const unsigned long long s = e[7 + t];
          if (s < bs) { bs = s; best[h] = 7 + t; }
        }
        if (best[h] >= 7) { const int w = g_fitw[h][best[h] - 7]; bset[h] = best[h] - 7; bw0[h] = (w & 255) - 128; bw1[h] = ((w >> 8) & 255) - 128; }
        else if (best[h] >= 4) { bset[h] = c_sgr_cand[best[h] - 4][0]; bw0[h] = c_sgr_cand[best[h] - 4][1]; bw1[h] = c_sgr_cand[best[h] - 4][2]; }
      }
      // the unit's record, by the lane of its first column in the first slice of the unit's first cell
      if (slice == 0 && cr == av1mi_lr_first_cell(ur, ush) && active && x == av1mi_lr_first_cell(unit, ush) * sh) {
        const unsigned long long *usse = unit_sse + (sse_base + unit) * 8;
        unsigned long long *e = F.err + (fit_base + unit) * AV1MI_LR_FIT_CANDS;
        for (int k = 0; k < 7; k++) e[k] = usse[k];
        for (int t = 0; t < AV1MI_LR_FIT_SETS; t++) if (g_fitw[hsel][t] < 0) e[7 + t] = ~0ull;   // absent (no slice reads these)
        int8_t *r = F.rec + (fit_base + unit) * 4;
        r[0] = (int8_t)best[hsel]; r[1] = (int8_t)bset[hsel]; r[2] = (int8_t)bw0[hsel]; r[3] = (int8_t)bw1[hsel];
        choice[sse_base + unit] = (uint8_t)best[hsel];
      }
    }
    for (int st = (y0 + so) / sh; st * sh - so < y1; st++) {
      const int s0 = st * sh - so, s1 = s0 + sh - 1;
      const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;   // <= 16 rows, ya even
      if constexpr (PHASE <= 2) {
        __syncthreads();
        lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, W, H, stride, lane);
        __syncthreads();
        int cur[16], sv[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int y = ya + i < yb ? ya + i : yb - 1;
          cur[i] = (int)g_win[y - ya + 3][lane + 3];
          sv[i] = active ? (int)src[(size_t)y * stride + x] : cur[i];
        }
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
                const int u = cur[i] << 4, s = (sv[i] << 4) - u;
                const int f0 = r0 ? fit_flt0(lane, ya + i, ya, cur[i]) - u : 0, f1 = r1 ? fit_flt1(lane, ya + i, ya, cur[i]) - u : 0;
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
            const int w = g_fitw[hsel][t], w0 = (w & 255) - 128, w1 = ((w >> 8) & 255) - 128;
            unsigned long long sse = 0;
#pragma unroll
            for (int i = 0; i < 16; i++)
              if (active && w >= 0 && ya + i < yb) {
                const int fl0 = r0 ? fit_flt0(lane, ya + i, ya, cur[i]) : 0, fl1 = r1 ? fit_flt1(lane, ya + i, ya, cur[i]) : 0;
                const int d = fit_blend(cur[i], r0, r1, fl0, fl1, w0, w1, maxv) - sv[i];
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
          lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, W, H, stride, lane);
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
                const int fl0 = r0 ? fit_flt0(lane, y, ya, c) : 0, fl1 = r1 ? fit_flt1(lane, y, ya, c) : 0;
                out[(size_t)y * stride + x] = (PIX)fit_blend(c, r0, r1, fl0, fl1, bw0[h], bw1[h], maxv);
              }
          }
        }
      }
    }
  }
  if constexpr (PHASE == 3) {
    // padding between the signalled and the coded size: copied with the last cell of the row / column (its last slice)
    const int py1 = (cr == crows - 1 && y1 == uy1) ? P.height >> sub : y1, px1 = last_col ? P.width >> sub : x1;
    for (int y = y0; y < py1; y++)
      for (int x = x0 + lane; x < px1; x += 64)
        if (y >= y1 || x >= x1) out[(size_t)y * stride + x] = cdef[(size_t)y * stride + x];
    if (!P.lr_chroma) {   // chroma is not restored: the luma blocks copy the co-located chroma
      const int cy0 = y0 >> 1, cy1 = py1 >> 1, cx0 = x0 >> 1, cx1 = px1 >> 1;
      for (int p = 0; p < 2; p++) {
        const size_t po = p ? P.plane_off_v : P.plane_off_u;
        for (int y = cy0; y < cy1; y++)
          for (int x = cx0 + lane; x < cx1; x += 64) out[po + (size_t)y * P.stride_c + x] = cdef[po + (size_t)y * P.stride_c + x];
      }
    }
  }
}

// PHASE 4: the bit strings of the self-guided units, fixed candidates included.  One thread per (frame, restored plane, tile) walks the
// tile's units in coding order - unit (r, c) of every plane is read with superblock (r << lr_unit_shift, c << lr_unit_shift), so a tile
// may start no unit - and carries the plane's RefSgrXqd, which starts every tile at Sgrproj_Xqd_Mid and takes every self-guided unit's
// weights, implied ones included.
__global__ void __launch_bounds__(64) lr_fit_code_kernel(Av1miDevParams P, Av1miLrFit F) {
  const int urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int nplanes = P.lr_chroma ? 3 : 1, tiles = P.tile_rows * P.tile_cols;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= P.n_frames * nplanes * tiles) return;
  const int tile = idx % tiles, pl = idx / tiles % nplanes, f = idx / (tiles * nplanes);
  const int tr = tile / P.tile_cols, tc = tile % P.tile_cols, tsb = P.tile_sb;
  int ref0 = -32, ref1 = 31;
  for (int si = 0; si < tsb * tsb; si++) {
    const int sbr = tr * tsb + si / tsb, sbc = tc * tsb + si % tsb;
    const int ur = av1mi_lr_sb_unit(sbr, urows, P.lr_unit_shift), uc = av1mi_lr_sb_unit(sbc, ucols, P.lr_unit_shift);
    if (sbr >= P.sb_rows || sbc >= P.sb_cols || ur < 0 || uc < 0) continue;
    const size_t u = ((size_t)f * 3 + pl) * per + (size_t)ur * ucols + uc;
    const int8_t *r = F.rec + u * 4;
    if (r[0] < 4) continue;
    const Av1miBitString b = av1mi_lr_sgr_code(r[1], r[2], r[3], ref0, ref1);
    F.code[u * 2] = (uint32_t)b.bits; F.code[u * 2 + 1] = (uint32_t)b.len;
    ref0 = r[2]; ref1 = r[3];
  }
}

template <typename PIX>
void launch_fit_typed(const Av1miDevParams &R, int grid, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                      const unsigned long long *unit_sse, const Av1miLrFit &F, hipStream_t stream) {
  const PIX *a = (const PIX *)pre, *b = (const PIX *)cdef, *s = (const PIX *)src;
  PIX *o = (PIX *)out;
  hipLaunchKernelGGL((lr_fit_kernel<PIX, 1>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, choice, unit_sse, F);
  hipLaunchKernelGGL((lr_fit_kernel<PIX, 2>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, choice, unit_sse, F);
  hipLaunchKernelGGL((lr_fit_kernel<PIX, 3>), dim3(grid), dim3(64), 0, stream, R, a, b, s, o, choice, unit_sse, F);
}

}  // namespace

extern "C" hipError_t av1mi_launch_lr_fit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                          const unsigned long long *unit_sse, const Av1miLrFit *fit, int frame0, int count, hipStream_t stream) {
  const Av1miDevParams R = av1mi_frame_range(*P, frame0, count);
  const size_t upf = (size_t)av1mi_lr_frame_units(R), fit_upf = (size_t)3 * av1mi_lr_unit_rows(R) * av1mi_lr_unit_cols(R);
  pre = av1mi_frame_at(R, pre, frame0); cdef = av1mi_frame_at(R, cdef, frame0); src = av1mi_frame_at(R, src, frame0); out = av1mi_frame_at(R, out, frame0);
  choice += frame0 * upf; unit_sse += frame0 * upf * 8;
  Av1miLrFit F = *fit;
  F.sums += frame0 * fit_upf * AV1MI_LR_FIT_SETS * 5; F.err += frame0 * fit_upf * AV1MI_LR_FIT_CANDS; F.rec += frame0 * fit_upf * 4; F.code += frame0 * fit_upf * 2;
  const int grid = av1mi_lr_grid(R, count);   // == av1mi_launch_lr's
  if (R.bit_depth == 8) launch_fit_typed<uint8_t>(R, grid, pre, cdef, src, out, choice, unit_sse, F, stream);
  else launch_fit_typed<uint16_t>(R, grid, pre, cdef, src, out, choice, unit_sse, F, stream);
  const int threads = count * (R.lr_chroma ? 3 : 1) * R.tile_rows * R.tile_cols;
  hipLaunchKernelGGL(lr_fit_code_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, R, F);
  return hipGetLastError();
}
