// lr_kernel.hip - loop restoration: per-unit Wiener decision and filter on luma, and on chroma with
// enable_lr = 3 / 4.
//
// Replaces the restoration-filter search and application inside the SVT-AV1 worker behind `run_av1an`
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139).  Normative part: AV1 spec §7.17.3 (units offset by 8 luma
// rows), §7.17.4 (separable 7-tap Wiener filter, Round2 by 3 then 11, intermediate clamp) and §7.17.6 (rows outside the
// 64-row stripe come from the pre-CDEF frame, at most 2 rows away).  Encoder part: a unit takes the
// candidate filter with the smallest SSE against the source, or none; restated in oracle/av1o_lr.c.  With av1mi_params.enable_lr bits 14
// and 15 the smallest J = 16 SSE + lambda x side information instead (lr_rate_rule.h; no oracle).
//
// MI355X mapping: waves of 16 rows of a 64x64 unit (lane = column), two phases (see lr_unit_kernel).  Per stripe of the unit the horizontal pass of 70 rows goes to
// LDS as int16 (the spec's clamp keeps it in 16 bits for 8/10 bit), the vertical pass reads 7 LDS rows per sample.  The
// three candidates are evaluated for their SSE only (with enable_lr = 2 also three self-guided candidates: the A/B grids of
// both box-filter passes go to LDS per stripe section, see lr_pieces.h's box_grid); the winner is applied in a last pass that writes the final
// reconstruction (with enable_lr = 1 / 2 chroma is copied: FrameRestorationType = NONE; with 3 / 4 the chroma units are decided
// and filtered in the same two launches, see lr_chroma).  Algorithmic HBM bytes: CDEF frame read + pre-CDEF rows at stripe edges
// + source read + final write = ~3*L*b + N*b per frame (~3*N*b with the chroma units).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "lr_rate_rule.h"

namespace {

#include "lr_pieces.h"   // candidate tables, LDS tiles, the staged window, both filters, the decision, the tail, LR_SLICES / LR_SLICES_C

// the self-guided candidates: lr_pieces.h's box filter with the strengths of their set as compile-time constants
constexpr int kSgrEps0 = av1mi_sgr_eps0(AV1MI_SGR_CAND_SET), kSgrEps1 = av1mi_sgr_eps1(AV1MI_SGR_CAND_SET);
static_assert(av1mi_sgr_r0(AV1MI_SGR_CAND_SET) == 2 && av1mi_sgr_r1(AV1MI_SGR_CAND_SET) == 1, "the candidates' set has both radii");
// both grids of a section, see box_grid (their readers wait at the caller's barrier)
__device__ __forceinline__ void sgr_grids(int bd, int ya, int yb, int lane) {
  box_grid<0>(bd, ya, yb, lane, kSgrEps0);
  box_grid<1>(bd, ya, yb, lane, kSgrEps1);
}
// the two box-filter outputs of sample (xs + lane, y), and candidate k's blend of them: the candidates differ only in the blend
__device__ __forceinline__ void box_flt01(int lane, int y, int ya, int cur, int &f0, int &f1) { f1 = box_flt1(lane, y, ya, cur); f0 = box_flt0(lane, y, ya, cur); }
__device__ __forceinline__ int sgr_cand(int k, int cur, int f0, int f1, int maxv) {
  return box_blend(cur, 1, 1, f0, f1, c_sgr_cand[k][1], c_sgr_cand[k][2], maxv);
}

// ---- chroma units (enable_lr = 3 / 4) ---------------------------------------------------------------------
// 32x32 units of the plane (lr_uv_shift 1), offset by 4 rows; stripes of 32 rows from 32 s - 4 (§7.17: StripeStartY = (64 s - 8) >> 1);
// the plane ends at Round2(signalled size, 1) - 1.  A wave takes up to 16 rows of two neighbouring units of one plane, lane = column:
// 64 lanes = 2 x 32 columns, so the window, the Wiener tile and the self-guided grids keep the luma layout (no LDS beyond luma's), and
// the sums and the decision stay per unit (lanes 0-31 / 32-63 of a pass).  The last unit of a row (up to 47 columns) is processed
// alone, or after its neighbour in a second pass of the wave.  Choices and sums are [frame][plane][unit].
// Larger units (lr_unit_shift, lr_geometry.h): the waves stay those of the 32x32 cells (crows x ccols of them); a cell's sums go to the unit it
// lies in and its rows take that unit's decision.  The two halves of a wave may then be one unit: two atomics to one address.
template <typename PIX, bool SGR, int PHASE>
__device__ __forceinline__ void lr_chroma(const Av1miDevParams &P, int item, const PIX *pre, const PIX *cdef, const PIX *src, PIX *out,
                                          uint8_t *choice, unsigned long long *unit_sse, int crows, int ccols) {
  const int pairs = (ccols + 1) >> 1, slice = item % LR_SLICES_C, rest = item / LR_SLICES_C;
  const int pc = rest % pairs, cr = rest / pairs % crows, pl = rest / (pairs * crows) % 2, f = rest / (pairs * crows * 2);
  const int ush = P.lr_unit_shift, urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), ur = av1mi_lr_unit_of_cell(cr, urows, ush);
  const int lane = threadIdx.x;
  const size_t fo = (size_t)f * P.frame_samples + (pl ? P.plane_off_v : P.plane_off_u);
  pre += fo; cdef += fo; src += fo; out += fo;
  const int W = (P.true_w + 1) >> 1, H = (P.true_h + 1) >> 1, stride = P.stride_c;
  const int uy0 = av1mi_lr_row0(cr, 0, 1), uy1 = av1mi_lr_row1(cr, crows, 0, 1, H);   // the cell row's rows
  const int y0 = uy0 + slice * 16, y1 = y0 + 16 < uy1 ? y0 + 16 : uy1;              // this wave's rows
  if (y0 >= uy1) return;
  const int x0 = pc * 64, x1 = pc == pairs - 1 ? W : x0 + 64;
  const int maxv = (1 << P.bit_depth) - 1;
  const size_t ubase = ((size_t)f * 3 + 1 + pl) * urows * ucols + (size_t)ur * ucols;   // unit (ur, 0) of the plane
  for (int xs = x0; xs < x1; xs += 64) {
    const int x = xs + lane;
    const bool active = x < x1;
    const int uc_lo = av1mi_lr_unit_of_cell(min(ccols - 1, xs >> 5), ucols, ush), uc_hi = av1mi_lr_unit_of_cell(min(ccols - 1, (xs >> 5) + 1), ucols, ush);
    const int uc = lane < 32 ? uc_lo : uc_hi;
    if constexpr (PHASE == 0) {
      unsigned long long sse[7] = { 0, 0, 0, 0, 0, 0, 0 };
      for (int st = (y0 + 4) / 32; st * 32 - 4 < y1; st++) {
        const int s0 = st * 32 - 4, s1 = s0 + 31;
        const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;
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
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (ya + i < yb) { const int d = cur[i] - sv[i]; sse[0] += (unsigned long long)(d * d); }
        for (int k = 0; k < 3; k++) {
          int tf[7];
          taps_of_uv(k, tf);
          wiener_h(P.bit_depth, ya, yb, tf, lane);
#pragma unroll
          for (int i = 0; i < 16; i++)
            if (active && ya + i < yb) { const int d = wiener_v(i, lane, tf, maxv) - sv[i]; sse[k + 1] += (unsigned long long)(d * d); }
        }
        if constexpr (SGR) {
          sgr_grids(P.bit_depth, ya, yb, lane);
          __syncthreads();
#pragma unroll
          for (int i = 0; i < 16; i++)
            if (active && ya + i < yb) {
              int f0, f1;
              box_flt01(lane, ya + i, ya, cur[i], f0, f1);
#pragma unroll
              for (int k = 0; k < 3; k++) {
                const int d = sgr_cand(k, cur[i], f0, f1, maxv) - sv[i];
                sse[4 + k] += (unsigned long long)(d * d);
              }
            }
        }
      }
      for (int k = 0; k < (SGR ? 7 : 4); k++) {
        const unsigned long long v = half_sum64(sse[k]);
        if ((lane & 31) == 0 && v) atomicAdd(&unit_sse[(ubase + uc) * 8 + k], v);
      }
    } else {
      // both units' decisions in every lane (the stripe loop below stays uniform); each lane applies its own unit's
      unsigned long long bj;
      const LrRate rate = lr_rate(P, 1);
      const int best_lo = lr_decide(unit_sse + (ubase + uc_lo) * 8, SGR ? 6 : 3, rate, bj), best_hi = lr_decide(unit_sse + (ubase + uc_hi) * 8, SGR ? 6 : 3, rate, bj);
      const int best = lane < 32 ? best_lo : best_hi;
      if (slice == 0 && cr == av1mi_lr_first_cell(ur, ush) && x == av1mi_lr_first_cell(uc, ush) * 32) choice[ubase + uc] = (uint8_t)best;
      const bool any_wiener = (best_lo && best_lo <= 3) || (best_hi && best_hi <= 3), any_sgr = best_lo > 3 || best_hi > 3;
      int tf[7];
      taps_of_uv(best && best <= 3 ? best - 1 : 0, tf);
      for (int st = (y0 + 4) / 32; st * 32 - 4 < y1; st++) {
        const int s0 = st * 32 - 4, s1 = s0 + 31;
        const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;
        if (any_wiener || any_sgr) {
          __syncthreads();
          lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, W, H, stride, lane);
          __syncthreads();
        }
        if constexpr (SGR) {
          if (any_sgr) {
            sgr_grids(P.bit_depth, ya, yb, lane);
            __syncthreads();
          }
        }
        if (any_wiener) wiener_h(P.bit_depth, ya, yb, tf, lane);   // per-lane taps; g_mid is private to the lane's column
        if (active)
          for (int y = ya; y < yb; y++) {
            int v;
            if (best > 3) {
              const int cur = (int)g_win[y - ya + 3][lane + 3];
              int f0, f1;
              box_flt01(lane, y, ya, cur, f0, f1);
              v = sgr_cand(best - 4, cur, f0, f1, maxv);
            } else if (best) {
              v = wiener_v(y - ya, lane, tf, maxv);
            } else {
              v = cdef[(size_t)y * stride + x];
            }
            out[(size_t)y * stride + x] = (PIX)v;
          }
      }
    }
  }
  if constexpr (PHASE == 1) lr_tail<PIX>(P, cdef, out, 1, false, cr == crows - 1 && y1 == uy1, pc == pairs - 1, x0, x1, y0, y1, stride, lane);
}

// A unit is LR_SLICES waves, one per 16 of its rows (the last unit of a column has up to 103), in two launches: PHASE 0 adds
// the slice's SSE of every candidate to the unit's sums (atomics), PHASE 1 reads the sums, takes the same decision in every
// slice and applies it to its rows.  (As one wave per unit the kernel took 221 us of an inter frame's serial chain.)
// Larger units (lr_unit_shift): the blocks stay those of the 64x64 cells; the sums and the decision are those of the unit a cell lies in.
// CHROMA (enable_lr = 3 / 4): the grid's luma blocks are followed by the chroma units' (lr_chroma), and choices and sums are
// [frame][plane][unit]; without it they are [frame][unit] and the luma blocks copy the co-located chroma.
template <typename PIX, bool SGR, bool CHROMA, int PHASE>
__global__ void __launch_bounds__(64) lr_unit_kernel(Av1miDevParams P, const PIX *__restrict__ pre, const PIX *__restrict__ cdef,
                                                    const PIX *__restrict__ src, PIX *__restrict__ out, uint8_t *__restrict__ choice,
                                                    unsigned long long *__restrict__ unit_sse /* [frame][(plane)][unit][8] */) {
  // units and stripes follow the signalled size; the last unit of a row/column also carries the padding up to the coded
  // size (copied, never filtered), so the whole frame buffer is defined
  const int crows = av1mi_lr_cell_rows(P), ccols = av1mi_lr_cell_cols(P), per_frame = crows * ccols;
  const int ush = P.lr_unit_shift, urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P);
  if constexpr (CHROMA) {
    const int luma_blocks = P.n_frames * per_frame * LR_SLICES;
    if ((int)blockIdx.x >= luma_blocks) {
      lr_chroma<PIX, SGR, PHASE>(P, (int)blockIdx.x - luma_blocks, pre, cdef, src, out, choice, unit_sse, crows, ccols);
      return;
    }
  }
  const int item = blockIdx.x / LR_SLICES, slice = blockIdx.x % LR_SLICES;
  const int f = item / per_frame, cell = item % per_frame, cr = cell / ccols, cc = cell % ccols;
  const int ur = av1mi_lr_unit_of_cell(cr, urows, ush), uc = av1mi_lr_unit_of_cell(cc, ucols, ush);
  const int uidx = f * (CHROMA ? 3 : 1) * urows * ucols + ur * ucols + uc;   // the unit's choice and sums
  const int lane = threadIdx.x;
  const size_t fo = (size_t)f * P.frame_samples;
  pre += fo; cdef += fo; src += fo; out += fo;
  const int uy0 = av1mi_lr_row0(cr, 0, 0), uy1 = av1mi_lr_row1(cr, crows, 0, 0, P.true_h);   // the cell's rows
  const int y0 = uy0 + slice * 16, y1 = y0 + 16 < uy1 ? y0 + 16 : uy1;                      // this wave's rows
  if (y0 >= uy1) return;
  const int x0 = cc * 64, x1 = cc == ccols - 1 ? P.true_w : x0 + 64;
  const int maxv = (1 << P.bit_depth) - 1;
  unsigned long long *usse = unit_sse + (size_t)uidx * 8;
  if constexpr (PHASE == 0) {
  // ---- SSE without restoration and with each candidate
  unsigned long long sse[7] = { 0, 0, 0, 0, 0, 0, 0 };
  for (int xs = x0; xs < x1; xs += 64) {
    const int x = xs + lane;
    const bool active = x < x1;
    for (int st = (y0 + 8) / 64; st * 64 - 8 < y1; st++) {
      const int s0 = st * 64 - 8, s1 = s0 + 63;
      const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;
      __syncthreads();
      lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, P.true_w, P.true_h, P.stride_y, lane);   // the section's source window, once, for every candidate
      __syncthreads();
      int cur[16], sv[16];   // this lane's CDEF and source samples of the section (<= 16 rows)
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int y = ya + i < yb ? ya + i : yb - 1;
        cur[i] = (int)g_win[y - ya + 3][lane + 3];
        sv[i] = active ? (int)src[(size_t)y * P.stride_y + x] : cur[i];
      }
#pragma unroll
      for (int i = 0; i < 16; i++)
        if (ya + i < yb) { const int d = cur[i] - sv[i]; sse[0] += (unsigned long long)(d * d); }
      for (int k = 0; k < 3; k++) {
        int tf[7];
        taps_of(k, tf);
        wiener_h(P.bit_depth, ya, yb, tf, lane);   // g_mid is private to the lane's column: no barrier needed
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (active && ya + i < yb) { const int d = wiener_v(i, lane, tf, maxv) - sv[i]; sse[k + 1] += (unsigned long long)(d * d); }
      }
      if constexpr (SGR) {
        sgr_grids(P.bit_depth, ya, yb, lane);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (active && ya + i < yb) {
            int f0, f1;
            box_flt01(lane, ya + i, ya, cur[i], f0, f1);
#pragma unroll
            for (int k = 0; k < 3; k++) {
              const int d = sgr_cand(k, cur[i], f0, f1, maxv) - sv[i];
              sse[4 + k] += (unsigned long long)(d * d);
            }
          }
      }
    }
  }
  for (int k = 0; k < (SGR ? 7 : 4); k++) {
    const unsigned long long v = wave_sum64(sse[k]);
    if (lane == 0 && v) atomicAdd(&usse[k], v);
  }
  } else {
  unsigned long long bj;
  const int best = lr_decide(usse, SGR ? 6 : 3, lr_rate(P, 0), bj);
  if (lane == 0 && slice == 0 && cr == av1mi_lr_first_cell(ur, ush) && cc == av1mi_lr_first_cell(uc, ush)) choice[uidx] = (uint8_t)best;
  // ---- apply: luma of the slice, and (without CHROMA) the co-located chroma (copied)
  for (int xs = x0; xs < x1; xs += 64) {
    const int x = xs + lane;
    const bool active = x < x1;
    for (int st = (y0 + 8) / 64; st * 64 - 8 < y1; st++) {
      const int s0 = st * 64 - 8, s1 = s0 + 63;
      const int ya = y0 > s0 ? y0 : s0, yb = y1 < s1 + 1 ? y1 : s1 + 1;
      if (best) {
        __syncthreads();
        lr_stage<PIX>(cdef, pre, xs, ya, yb, s0, s1, P.true_w, P.true_h, P.stride_y, lane);
        __syncthreads();
      }
      if (best > 3) {
        if constexpr (SGR) {
          sgr_grids(P.bit_depth, ya, yb, lane);
          __syncthreads();
          if (active)
            for (int y = ya; y < yb; y++) {
              const int cur = (int)g_win[y - ya + 3][lane + 3];
              int f0, f1;
              box_flt01(lane, y, ya, cur, f0, f1);
              out[(size_t)y * P.stride_y + x] = (PIX)sgr_cand(best - 4, cur, f0, f1, maxv);
            }
        }
      } else if (best) {
        int tf[7];
        taps_of(best - 1, tf);
        wiener_h(P.bit_depth, ya, yb, tf, lane);
        if (active)
          for (int y = ya; y < yb; y++) out[(size_t)y * P.stride_y + x] = (PIX)wiener_v(y - ya, lane, tf, maxv);
      } else if (active) {
        for (int y = ya; y < yb; y++) out[(size_t)y * P.stride_y + x] = cdef[(size_t)y * P.stride_y + x];
      }
    }
  }
  lr_tail<PIX>(P, cdef, out, 0, !CHROMA, cr == crows - 1 && y1 == uy1, cc == ccols - 1, x0, x1, y0, y1, P.stride_y, lane);
  }  // PHASE 1
}

// decide: 0 - phase 0 alone (the self-guided fit takes the decision, lr_fit_kernel.hip)
template <typename PIX, bool SGR, bool CHROMA>
void launch_lr_phases(const Av1miDevParams *P, int grid, const PIX *pre, const PIX *cdef, const PIX *src, PIX *out, uint8_t *choice,
                      unsigned long long *unit_sse, int decide, hipStream_t stream) {
  hipLaunchKernelGGL((lr_unit_kernel<PIX, SGR, CHROMA, 0>), dim3(grid), dim3(64), 0, stream, *P, pre, cdef, src, out, choice, unit_sse);
  if (decide) hipLaunchKernelGGL((lr_unit_kernel<PIX, SGR, CHROMA, 1>), dim3(grid), dim3(64), 0, stream, *P, pre, cdef, src, out, choice, unit_sse);
}

}  // namespace

extern "C" hipError_t av1mi_launch_lr(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                      unsigned long long *unit_sse, int clear, int decide, int frame0, int count, hipStream_t stream) {
  const LrLaunch L = lr_launch_head(P, pre, cdef, src, out, frame0, count);
  choice += L.unit0; unit_sse += L.unit0 * 8;
  if (clear) {
    hipError_t e = hipMemsetAsync(unit_sse, 0, count * L.upf * 8 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
  }
  // enable_lr = 2 (RESTORE_SWITCHABLE): the instantiations with the self-guided candidates (17 KB of LDS per wave, 6.2 KB without)
  lr_launch_typed(L, [&](auto *a, auto *b, auto *s, auto *o) {
    using PIX = std::remove_pointer_t<decltype(o)>;
    if (L.R.enable_lr == 2) {
      if (L.R.lr_chroma) launch_lr_phases<PIX, true, true>(&L.R, L.grid, a, b, s, o, choice, unit_sse, decide, stream);
      else launch_lr_phases<PIX, true, false>(&L.R, L.grid, a, b, s, o, choice, unit_sse, decide, stream);
    } else {
      if (L.R.lr_chroma) launch_lr_phases<PIX, false, true>(&L.R, L.grid, a, b, s, o, choice, unit_sse, decide, stream);
      else launch_lr_phases<PIX, false, false>(&L.R, L.grid, a, b, s, o, choice, unit_sse, decide, stream);
    }
  });
  return hipGetLastError();
}
