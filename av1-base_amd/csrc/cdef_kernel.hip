// cdef_kernel.hip - CDEF of the reconstructed frames: the filter, the strength search and the choice of the frame's strength set.
//
// Replaces the CDEF stage of the external SVT-AV1 worker behind `run_av1an` (av1an.rs:126-139):
// AV1 spec §7.15 - 8x8 direction search (§7.15.2) and the constrained primary/secondary filter (§7.15.3), 4:2:0, one strength set
// per frame (cdef_bits = 0) - or, with the strength search on, a set of up to 8 per frame and an index per superblock, chosen by
// cdef_search_kernel + cdef_select_kernel below.  The rules themselves - direction, strengths, taps, "not available", the sample
// filter, the search's candidates and pool - are cdef_pieces.h, which the host compiles too; this file is the MI355X mapping: one wave
// per 64x64 superblock (or per 8-row strip of it), each lane owns one 8x8 block for the direction search and one column for the filter.
// The superblock prelude stands in cdef_sb_body and again in cdef_search_kernel: as a function of its own it costs cdef_sb_kernel a
// register, and the filter is on a register cliff.
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "cdef_pieces.h"

namespace {

// CDEF reads the reconstruction straight from HBM/L2 through the vector L1 (every sample is touched ~5
// times by neighbouring lanes/rows of the same wave) and keeps only the per-8x8 decisions in LDS (256 B):
// the kernel can share a CU with the range-coding kernel, which holds 129 KB of LDS per CU.
struct CdefLds {
  uint8_t dir[64];       // luma direction of each 8x8 block
  uint8_t on[64];        // block is filtered
  uint16_t pri_y[64];    // variance-adjusted luma primary strength
};
__shared__ CdefLds g_cdef;

// The constrained filter (§7.15.3) of BR consecutive rows of one column (this lane's) whose 8x8 (4x4 chroma) block is the same
// for all of them: the direction - so the tap offsets - and the strengths are per-lane constants of the batch.  ALL loads of the
// batch (centre + 4 primary taps, + 8 secondary taps when SEC) are issued before anything is computed: the row-at-a-time form
// (load centre, branch on the block's filter flag, load taps, filter, store) paid two memory latencies per row - 192 per
// superblock, ~600 k cycles per wave with 73 % of them parked on loads.  No branches: a block that is not filtered runs with both
// strengths 0 (the filter then returns the sample itself), a tap outside the frame (EDGE superblocks only) is loaded from its
// clamped position and replaced by the centre sample ("not available", cdef_pieces.h).
// The loads take 32-bit sample indices from the (wave-uniform) plane pointer (av1mi_cdef_ld): scalar base + 32-bit offset
// instead of a 64-bit address pair per tap.
template <typename PIX>
__device__ __forceinline__ void st_px(PIX *pl, int idx, int v) {
  *reinterpret_cast<PIX *>(reinterpret_cast<char *>(pl) + (unsigned)idx * (unsigned)sizeof(PIX)) = (PIX)v;
}
template <typename PIX, bool EDGE, bool SEC, int BR>
__device__ __forceinline__ void cdef_rows(const PIX *pl, PIX *out, int stride, int w, int h, int gx, int gy0, int pri, int sec, int pri_shift,
                                          int sec_shift, int dir, int coeff_shift, const PIX *srcp = nullptr, unsigned *acc = nullptr) {
  constexpr int NT = SEC ? 12 : 4;
  int ty[NT], tx[NT], toff[NT];
  av1mi_cdef_tap_offsets<NT>(dir, ty, tx);
#pragma unroll
  for (int k = 0; k < NT; k++) toff[k] = ty[k] * stride + tx[k];
  int c[BR], t[BR][NT];
  unsigned okm[BR];   // EDGE: bit k = tap k of the row is inside the frame
#pragma unroll
  for (int r = 0; r < BR; r++) {
    const int gy = EDGE ? (gy0 + r < h ? gy0 + r : h - 1) : gy0 + r;   // (rows below a partial superblock: loaded from the last row, never stored)
    const int base = gy * stride + gx;
    c[r] = av1mi_cdef_ld(pl, base);
    okm[r] = 0;
#pragma unroll
    for (int k = 0; k < NT; k++) {
      if (EDGE) {
        int yy, xx;
        okm[r] |= (unsigned)av1mi_cdef_tap_pos(gy, gx, ty[k], tx[k], w, h, &yy, &xx) << k;
        t[r][k] = av1mi_cdef_ld(pl, yy * stride + xx);
      } else {
        t[r][k] = av1mi_cdef_ld(pl, base + toff[k]);
      }
    }
  }
  const int odd = (pri >> coeff_shift) & 1;
#pragma unroll
  for (int r = 0; r < BR; r++) {
    // av1mi_cdef_sample's loop, kept in place: through the piece the SEC instantiations spill up to 84 bytes per lane more
    const int x = c[r];
    int sum = 0, mx = x, mn = x;
#pragma unroll
    for (int k = 0; k < NT; k++) {
      const int p = (EDGE && !((okm[r] >> k) & 1)) ? x : t[r][k];
      sum += av1mi_cdef_tap_weight(k, odd) * (k < 4 ? av1mi_cdef_constrain(p - x, pri, pri_shift) : av1mi_cdef_constrain(p - x, sec, sec_shift));
      mx = p > mx ? p : mx;
      mn = p < mn ? p : mn;
    }
    const int v = av1mi_cdef_finish(x, sum, mn, mx);
    if (!EDGE || gy0 + r < h) {
      st_px(out, (gy0 + r) * stride + gx, v);
      // (chunk-wide launches: the squared error against the source is summed here - sse_kernel's second pass over the frames would
      // end after the range coder that CDEF runs beside)
      if (acc) { const int d = v - av1mi_cdef_ld(srcp, (gy0 + r) * stride + gx); *acc += (unsigned)(d * d); }
    }
  }
}

template <typename PIX, bool EDGE, bool SEC, bool SSEV>
__device__ __forceinline__ void cdef_filter_sb(const Av1miDevParams &P, const PIX *fr, PIX *fo, int x0, int y0, int w, int h, int lane,
                                               int row0, int row1 /* luma rows [row0, row1) of the superblock, multiples of 8 */,
                                               const PIX *sf /* SSEV: the source frame */, unsigned long long *sse_f /* SSEV: the frame's three sums */) {
  const int coeff_shift = P.bit_depth - 8;
  // ---- luma: lane = column, batches of the 8 rows of a block row (row-contiguous HBM loads and stores)
  {
    const int sec = av1mi_cdef_sec_strength(P.cdef_y_sec, coeff_shift);
    const int damping = P.cdef_damping + coeff_shift;
    const int sec_shift = av1mi_cdef_damp_shift(sec, damping);
    unsigned acc = 0, *const accp = SSEV ? &acc : nullptr;
    if (lane < w) {
      for (int r = row0; r < (row1 < h ? row1 : h); r += 8) {
        const int b = (r >> 3) * 8 + (lane >> 3);
        const bool on = g_cdef.on[b] != 0;
        const int pri = on ? (int)g_cdef.pri_y[b] : 0, sec_b = on ? sec : 0;
        const int dir = P.cdef_y_pri == 0 ? 0 : g_cdef.dir[b];
        // batches: 8 rows with primary taps only in interior superblocks; 4 rows with the secondary taps or the frame-edge tests
        if (SEC && sec) {
          cdef_rows<PIX, EDGE, true, 4>(fr, fo, P.stride_y, P.width, P.height, x0 + lane, y0 + r, pri, sec_b, av1mi_cdef_damp_shift(pri, damping), sec_shift, dir, coeff_shift, sf, accp);
          cdef_rows<PIX, EDGE, true, 4>(fr, fo, P.stride_y, P.width, P.height, x0 + lane, y0 + r + 4, pri, sec_b, av1mi_cdef_damp_shift(pri, damping), sec_shift, dir, coeff_shift, sf, accp);
        } else if (EDGE) {
          cdef_rows<PIX, true, false, 4>(fr, fo, P.stride_y, P.width, P.height, x0 + lane, y0 + r, pri, 0, av1mi_cdef_damp_shift(pri, damping), 0, dir, coeff_shift, sf, accp);
          cdef_rows<PIX, true, false, 4>(fr, fo, P.stride_y, P.width, P.height, x0 + lane, y0 + r + 4, pri, 0, av1mi_cdef_damp_shift(pri, damping), 0, dir, coeff_shift, sf, accp);
        } else {
          cdef_rows<PIX, false, false, 8>(fr, fo, P.stride_y, P.width, P.height, x0 + lane, y0 + r, pri, 0, av1mi_cdef_damp_shift(pri, damping), 0, dir, coeff_shift, sf, accp);
        }
      }
    }
    if constexpr (SSEV) {
      unsigned long long t = acc;
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0 && t) atomicAdd(&sse_f[0], t);
    }
  }
  // ---- chroma: lanes 0-31 = columns of U, lanes 32-63 = columns of V; batches of the 4 rows of a block row
  {
    const int pl = lane >> 5, col = lane & 31;
    const PIX *cp = fr + (pl ? P.plane_off_v : P.plane_off_u);
    PIX *op = fo + (pl ? P.plane_off_v : P.plane_off_u);
    const int pri0 = P.cdef_uv_pri << coeff_shift;
    const int sec0 = av1mi_cdef_sec_strength(P.cdef_uv_sec, coeff_shift);
    const int damping = P.cdef_damping + coeff_shift - 1;
    const int pri_shift = av1mi_cdef_damp_shift(pri0, damping), sec_shift = av1mi_cdef_damp_shift(sec0, damping);
    const int wc = w >> 1, hc = h >> 1;
    const PIX *sp = SSEV ? sf + (pl ? P.plane_off_v : P.plane_off_u) : nullptr;
    unsigned acc = 0, *const accp = SSEV ? &acc : nullptr;
    if (col < wc) {
      for (int r = row0 >> 1; r < ((row1 >> 1) < hc ? (row1 >> 1) : hc); r += 4) {
        const int b = (r >> 2) * 8 + (col >> 2);
        const bool on = g_cdef.on[b] != 0;
        const int pri = on ? pri0 : 0, sec = on ? sec0 : 0;
        const int dir = pri0 == 0 ? 0 : (int)g_cdef.dir[b];
        if (SEC && sec0) cdef_rows<PIX, EDGE, true, 4>(cp, op, P.stride_c, P.width >> 1, P.height >> 1, (x0 >> 1) + col, (y0 >> 1) + r, pri, sec, pri_shift, sec_shift, dir, coeff_shift, sp, accp);
        else cdef_rows<PIX, EDGE, false, 4>(cp, op, P.stride_c, P.width >> 1, P.height >> 1, (x0 >> 1) + col, (y0 >> 1) + r, pri, 0, pri_shift, 0, dir, coeff_shift, sp, accp);
      }
    }
    if constexpr (SSEV) {   // the two halves of the wave: U, V
      unsigned long long t = acc;
      for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if ((lane & 31) == 0 && t) atomicAdd(&sse_f[1 + pl], t);
    }
  }
}

// NS = 1: one wave per superblock (chunk-wide launches: throughput).  NS = 8: one wave per 8-row strip of a superblock
// (one-frame launches of inter chunks: NS x the waves and 1 / NS of the filter work per wave: latency).
// SEC: some secondary strength is non-zero (the default strengths have none: the instantiation without carries no secondary-tap code).
// SSEV: the squared error of the output against the source `src` is added to sse[frame][plane] (chunk-wide launches only).
// A superblock with nothing coded runs like the others, with every block off: strengths 0.
template <typename PIX, int NS, bool SEC, bool SSEV>
__device__ __forceinline__ void cdef_sb_body(const Av1miDevParams &P, const PIX *__restrict__ rec, PIX *__restrict__ fin,
                                             const Av1miBlkInfo *__restrict__ blk, const PIX *__restrict__ src, unsigned long long *__restrict__ sse,
                                             int f, int sb, int strip) {
  const int sbr = sb / P.sb_cols, sbc = sb % P.sb_cols;
  const int lane = threadIdx.x;
  const PIX *fr = rec + (size_t)f * P.frame_samples;
  PIX *fo = fin + (size_t)f * P.frame_samples;
  const int x0 = sbc * 64, y0 = sbr * 64;
  const int coeff_shift = P.bit_depth - 8;
  const int w = P.width - x0 < 64 ? P.width - x0 : 64, h = P.height - y0 < 64 ? P.height - y0 : 64;
  // ---- per-8x8 decisions: lane = 8x8 block
  const int b8r = lane >> 3, b8c = lane & 7;
  const bool inside = (sbr * 8 + b8r) < P.b8_rows && (sbc * 8 + b8c) < P.b8_cols;
  int skip = 1;
  if (inside) skip = blk[(size_t)f * P.b8_rows * P.b8_cols + (size_t)(sbr * 8 + b8r) * P.b8_cols + sbc * 8 + b8c].skip;
  // cdef_idx of the superblock is coded (== 0) iff some block in it is not skipped (§5.11.56)
  const bool sb_on = __ballot(inside && !skip) != 0ull;
  const bool do_filter = P.enable_cdef && sb_on && inside && !skip;
  const bool mine = NS == 1 || b8r / (8 / NS) == strip;   // this wave decides (and filters) only the blocks of its strip
  {
    int ydir = 0, var = 0;
    if (do_filter && mine) {
      // direction search §7.15.2 on the block's 8 rows of 8 samples (one-frame launches of inter chunks: the lane reads its block
      // from L1/L2; the second group's reads hit L1)
      const PIX *ty = fr + (size_t)(y0 + b8r * 8) * P.stride_y + x0 + b8c * 8;
      int px[8][8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = 0; j < 8; j++) px[i][j] = ((int)ty[(size_t)i * P.stride_y + j] >> coeff_shift) - 128;
      }
      av1mi_cdef_direction_8x8(px, ydir, var);
    }
    const int pri = av1mi_cdef_adjusted_pri(P.cdef_y_pri, var, coeff_shift);
    g_cdef.dir[lane] = (uint8_t)ydir;
    g_cdef.on[lane] = (uint8_t)do_filter;
    g_cdef.pri_y[lane] = (uint16_t)pri;
  }
  __syncthreads();
  // taps reach 2 samples beyond the superblock (1 in chroma): interior superblocks need no tests
  const bool edge = x0 < 2 || y0 < 2 || x0 + 66 > P.width || y0 + 66 > P.height;
  const int row0 = NS == 1 ? 0 : strip * (64 / NS), row1 = NS == 1 ? 64 : (strip + 1) * (64 / NS);
  const PIX *sf = SSEV ? src + (size_t)f * P.frame_samples : nullptr;
  unsigned long long *sse_f = SSEV ? sse + (size_t)f * 3 : nullptr;
  if (edge) cdef_filter_sb<PIX, true, SEC, SSEV>(P, fr, fo, x0, y0, w, h, lane, row0, row1, sf, sse_f);
  else cdef_filter_sb<PIX, false, SEC, SSEV>(P, fr, fo, x0, y0, w, h, lane, row0, row1, sf, sse_f);
}

// SEL: the strength search is on - each superblock filters with the pair its frame's set assigns it (P.cdef_idx / P.cdef_sel, frame-relative
// like `rec`), loaded once per wave; the fixed-strength instantiations (SEL = false) are what they were before the search existed.
template <typename PIX, int NS, bool SEC, bool SSEV = false, bool SEL = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) cdef_sb_kernel(Av1miDevParams P, const PIX *__restrict__ rec, PIX *__restrict__ fin,
                                                    const Av1miBlkInfo *__restrict__ blk,
                                                    const PIX *__restrict__ src = nullptr, unsigned long long *__restrict__ sse = nullptr) {
  const int sbs_per_frame = P.sb_rows * P.sb_cols;
  const int strip = NS == 1 ? 0 : (int)(blockIdx.x % NS);
  const int item = blockIdx.x / NS;
  const int f = item / sbs_per_frame, sb = item % sbs_per_frame;
  if constexpr (SEL) {
    Av1miDevParams Q = P;
    const int ci = P.cdef_idx[(size_t)f * sbs_per_frame + sb];   // -1: no block of the superblock is coded, nothing is filtered
    const Av1miCdefStrengths s = av1mi_cdef_pair_strengths(ci >= 0 ? (int)P.cdef_sel[f * 8 + ci] : 0);
    Q.cdef_y_pri = s.y_pri; Q.cdef_y_sec = s.y_sec; Q.cdef_uv_pri = s.uv_pri; Q.cdef_uv_sec = s.uv_sec;
    cdef_sb_body<PIX, NS, SEC, SSEV>(Q, rec, fin, blk, src, sse, f, sb, strip);
  } else {
    cdef_sb_body<PIX, NS, SEC, SSEV>(P, rec, fin, blk, src, sse, f, sb, strip);
  }
}

// ------------------------------------------------------------------------------ CDEF strength search
// Per superblock the squared error against the source of the CDEF output under every candidate of the pool: 16 luma candidates
// (err[0 .. 15]) and 8 chroma candidates (err[16 .. 23], U + V), counted over the signalled frame size only.  The prelude is
// cdef_sb_kernel's; what a candidate makes of a sample is av1mi_cdef_search_luma / _chroma (cdef_pieces.h).  Unfiltered (skipped)
// blocks add the same error to every candidate.  Per lane in 32 bits (<= 64 samples of <= 1023^2), per
// wave through LDS in 64 bits, into the table with 64-bit atomics (integer sums: the order does not matter).
// NS: strips per superblock as cdef_sb_kernel (NS = 8 for one-frame launches on the P-frame chain).  Superblocks whose blocks are all
// skipped code no cdef_idx: -1 is written for them (0 for the others, cdef_select_kernel fills in the index) and their errors stay 0.
struct CdefSearchLds {
  uint8_t dir[64];
  uint8_t on[64];
  int var[64];
  uint32_t acc[24][65];
};
__shared__ CdefSearchLds g_cs;

// one plane's columns: NC candidates from acc[C0] on; sub = 0: luma (lane = column), 1: chroma (lanes 0-31 = U, 32-63 = V)
template <typename PIX, bool EDGE, int sub>
__device__ __forceinline__ void cdef_search_plane(const Av1miDevParams &P, const PIX *pl, const PIX *sp, int sx0, int sy0, int sw, int sh, int row0, int row1, int col, uint32_t *acc) {
  constexpr int NC = sub ? 8 : 16;
  const int coeff_shift = P.bit_depth - 8, damping = P.cdef_damping + coeff_shift - sub;
  const int stride = sub ? P.stride_c : P.stride_y, pw = P.width >> sub, ph = P.height >> sub;
  const int x0 = sx0 >> sub, y0 = sy0 >> sub, w = sw >> sub, h = sh >> sub, r1 = row1 >> sub;
  const int tw = (P.true_w >> sub) - x0, th = (P.true_h >> sub) - y0;   // counted region (signalled size), superblock-relative
  uint32_t base = 0;
  if (col < w && col < tw) {
    for (int r = row0 >> sub; r < (r1 < h ? r1 : h) && r < th; r++) {
      const int b = (r >> (3 - sub)) * 8 + (col >> (3 - sub));
      const int gx = x0 + col, gy = y0 + r;
      const int x = av1mi_cdef_ld(pl, gy * stride + gx), s = av1mi_cdef_ld(sp, gy * stride + gx);
      if (!g_cs.on[b]) { base += (uint32_t)((x - s) * (x - s)); continue; }
      int v[NC];
      if constexpr (sub == 0) av1mi_cdef_search_luma<PIX, EDGE>(pl, stride, pw, ph, gy, gx, x, g_cs.dir[b], g_cs.var[b], coeff_shift, damping, v);
      else av1mi_cdef_search_chroma<PIX, EDGE>(pl, stride, pw, ph, gy, gx, x, g_cs.dir[b], coeff_shift, damping, v);
#pragma unroll
      for (int k = 0; k < NC; k++) acc[k] += (uint32_t)((v[k] - s) * (v[k] - s));
    }
  }
#pragma unroll
  for (int k = 0; k < NC; k++) acc[k] += base;
}

template <typename PIX, bool EDGE>
__device__ __forceinline__ void cdef_search_sb(const Av1miDevParams &P, const PIX *fr, const PIX *sf, int x0, int y0, int w, int h, int lane,
                                               int row0, int row1, uint32_t (&acc)[24]) {
  cdef_search_plane<PIX, EDGE, 0>(P, fr, sf, x0, y0, w, h, row0, row1, lane, acc);
  const long off = (lane >> 5) ? P.plane_off_v : P.plane_off_u;
  cdef_search_plane<PIX, EDGE, 1>(P, fr + off, sf + off, x0, y0, w, h, row0, row1, lane & 31, acc + 16);
}

template <typename PIX, int NS>
__global__ void __launch_bounds__(64) cdef_search_kernel(Av1miDevParams P, int frame0, const PIX *__restrict__ rec, const PIX *__restrict__ src,
                                                         const Av1miBlkInfo *__restrict__ blk) {
  // (cdef_sb_body's prelude, but for the early exit and what is kept: the variance, not the strength)
  const int sbs_per_frame = P.sb_rows * P.sb_cols;
  const int strip = NS == 1 ? 0 : (int)(blockIdx.x % NS);
  const int item = blockIdx.x / NS;
  const int f = frame0 + item / sbs_per_frame, sb = item % sbs_per_frame;
  const int sbr = sb / P.sb_cols, sbc = sb % P.sb_cols;
  const int lane = threadIdx.x;
  const PIX *fr = rec + (size_t)f * P.frame_samples, *sf = src + (size_t)f * P.frame_samples;
  const int x0 = sbc * 64, y0 = sbr * 64;
  const int coeff_shift = P.bit_depth - 8;
  const int w = P.width - x0 < 64 ? P.width - x0 : 64, h = P.height - y0 < 64 ? P.height - y0 : 64;
  const int b8r = lane >> 3, b8c = lane & 7;
  const bool inside = (sbr * 8 + b8r) < P.b8_rows && (sbc * 8 + b8c) < P.b8_cols;
  int skip = 1;
  if (inside) skip = blk[(size_t)f * P.b8_rows * P.b8_cols + (size_t)(sbr * 8 + b8r) * P.b8_cols + sbc * 8 + b8c].skip;
  const bool sb_on = __ballot(inside && !skip) != 0ull;
  if (strip == 0 && lane == 0) P.cdef_idx[(size_t)f * sbs_per_frame + sb] = sb_on ? 0 : -1;
  if (!sb_on) return;   // (wave-uniform)
  const bool do_filter = inside && !skip;
  const bool mine = NS == 1 || b8r / (8 / NS) == strip;
  {
    int ydir = 0, var = 0;
    if (do_filter && mine) {
      const PIX *ty = fr + (size_t)(y0 + b8r * 8) * P.stride_y + x0 + b8c * 8;
      int px[8][8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = 0; j < 8; j++) px[i][j] = ((int)ty[(size_t)i * P.stride_y + j] >> coeff_shift) - 128;
      }
      av1mi_cdef_direction_8x8(px, ydir, var);
    }
    g_cs.dir[lane] = (uint8_t)ydir;
    g_cs.on[lane] = (uint8_t)do_filter;
    g_cs.var[lane] = var;
  }
  __syncthreads();
  const bool edge = x0 < 2 || y0 < 2 || x0 + 66 > P.width || y0 + 66 > P.height;
  const int row0 = NS == 1 ? 0 : strip * (64 / NS), row1 = NS == 1 ? 64 : (strip + 1) * (64 / NS);
  uint32_t acc[24];
#pragma unroll
  for (int k = 0; k < 24; k++) acc[k] = 0;
  if (edge) cdef_search_sb<PIX, true>(P, fr, sf, x0, y0, w, h, lane, row0, row1, acc);
  else cdef_search_sb<PIX, false>(P, fr, sf, x0, y0, w, h, lane, row0, row1, acc);
  // per wave: transpose through LDS, 24 lanes sum a candidate's 64 lane sums in 64 bits
#pragma unroll
  for (int k = 0; k < 24; k++) g_cs.acc[k][lane] = acc[k];
  __syncthreads();
  if (lane < 24) {
    unsigned long long t = 0;
    for (int i = 0; i < 64; i++) t += g_cs.acc[lane][i];
    if (t) atomicAdd(&P.cdef_err[((size_t)f * sbs_per_frame + sb) * 24 + lane], t);
  }
}

// The frame's strength set and every superblock's index into it, one workgroup per frame: E[sb][p] =
// err[sb][l] + err[sb][16 + c] for pair p = 8 l + c.  n = 2^cdef_bits greedy picks (each minimising the sum over superblocks of the best
// error so far), then two refinement passes that replace S[j] by the pair minimising the sum against the other n - 1 when that is strictly
// lower; first minimum in p order on ties.  Then cdef_idx = the first j minimising E[sb][S[j]] on coded superblocks, the set into
// cdef_sel, and the 12 n strength bits into the frame's header slot (the host wrote placeholders of that length at cdef_str_bit).
// Threads: 128 pairs x 4 quarters of the superblocks.
__global__ void __launch_bounds__(512) cdef_select_kernel(Av1miDevParams P, int frame0, uint8_t *__restrict__ hdr_blob) {
  __shared__ unsigned long long part[512];
  __shared__ int S[8];
  __shared__ int best_p;
  const int f = frame0 + (int)blockIdx.x, t = threadIdx.x, p = t & 127, q = t >> 7;
  const int nsb = P.sb_rows * P.sb_cols, n = 1 << P.cdef_bits;
  const unsigned long long *E = P.cdef_err + (size_t)f * nsb * 24;
  const int8_t *idx = P.cdef_idx + (size_t)f * nsb;
  const int pl = av1mi_cdef_pair_luma_at(p), pc = av1mi_cdef_pair_chroma_at(p);   // this thread's pair, out of the loops
  // cost of every pair against the set S[0 .. m) without entry `excl` (-1: none); leaves the argmin in best_p, the costs in part[0 .. 128)
  auto pass = [&](int m, int excl) {
    unsigned long long sum = 0;
    for (int sb = q; sb < nsb; sb += 4) {
      if (idx[sb] < 0) continue;   // no cdef_idx coded: the same error under every pair
      const unsigned long long *e = E + (size_t)sb * 24;
      unsigned long long o = ~0ull;
      for (int i = 0; i < m; i++)
        if (i != excl) { const unsigned long long v = av1mi_cdef_pair_err(e, S[i]); o = v < o ? v : o; }
      const unsigned long long v = e[pl] + e[pc];
      sum += v < o ? v : o;
    }
    part[t] = sum;
    __syncthreads();
    if (t < 128) part[t] = part[t] + part[t + 128] + part[t + 256] + part[t + 384];
    __syncthreads();
    if (t == 0) {
      int b = 0;
      for (int i = 1; i < 128; i++) if (part[i] < part[b]) b = i;
      best_p = b;
    }
    __syncthreads();
  };
  for (int m = 0; m < n; m++) {
    pass(m, -1);
    if (t == 0) S[m] = best_p;
    __syncthreads();
  }
  if (n > 1)
    for (int it = 0; it < 2; it++)
      for (int j = 0; j < n; j++) {
        pass(n, j);
        if (t == 0 && part[best_p] < part[S[j]]) S[j] = best_p;
        __syncthreads();
      }
  for (int sb = t; sb < nsb; sb += 512) {
    if (idx[sb] < 0) continue;
    const unsigned long long *e = E + (size_t)sb * 24;
    int bj = 0;
    unsigned long long bv = ~0ull;
    for (int j = 0; j < n; j++) { const unsigned long long v = av1mi_cdef_pair_err(e, S[j]); if (v < bv) { bv = v; bj = j; } }
    P.cdef_idx[(size_t)f * nsb + sb] = (int8_t)bj;
  }
  if (t < n) P.cdef_sel[f * 8 + t] = (uint8_t)S[t];
  if (t == 0) {   // the 12 strength bits of every pair of the set
    uint8_t *h = hdr_blob + P.seq_hdr_bytes + (size_t)f * P.hdr_slot_bytes;
    int bit = P.cdef_str_bit[av1mi_frame_is_inter(P, f)];
    for (int j = 0; j < n; j++) {
      const uint32_t v = av1mi_cdef_pair_bits(S[j]);
      for (int k = 11; k >= 0; k--, bit++) {
        const uint8_t m = (uint8_t)(0x80 >> (bit & 7));
        h[bit >> 3] = ((v >> k) & 1) ? (uint8_t)(h[bit >> 3] | m) : (uint8_t)(h[bit >> 3] & ~m);
      }
    }
  }
}

}  // namespace

extern "C" hipError_t av1mi_launch_cdef(const Av1miDevParams *P, const void *rec, void *fin, const Av1miBlkInfo *blk, const void *src,
                                        unsigned long long *sse, int frame0, int count, hipStream_t stream) {
  const Av1miDevParams R = av1mi_frame_range(*P, frame0, count);
  rec = av1mi_frame_at(R, rec, frame0); fin = av1mi_frame_at(R, fin, frame0); blk += (size_t)frame0 * R.b8_rows * R.b8_cols;
  if (src) src = av1mi_frame_at(R, src, frame0);
  if (sse) sse += (size_t)frame0 * 3;
  const int grid = count * R.sb_rows * R.sb_cols;
  const bool strips = count == 1;  // a one-frame launch sits on an inter chunk's serial chain
  const bool sel = R.cdef_search != 0;   // the search's pairs: some may have a secondary strength (the SEC kernels branch per superblock)
  const bool sec = sel || R.cdef_y_sec != 0 || R.cdef_uv_sec != 0;
  const bool sse_here = src || sse;
  if (sse_here && (strips || !src || !sse)) return hipErrorInvalidValue;
  if (sel && (!R.cdef_idx || !R.cdef_sel)) return hipErrorInvalidValue;
  // one-frame launches: 8-row strips (4 080 waves at 1080p, still one round of the chip) - 16-row strips were 2.5 us per frame slower
#define CDEF_LAUNCH2(PIXT, SECV, SELV)                                                                                                     \
  do {                                                                                                                                     \
    if (strips) hipLaunchKernelGGL((cdef_sb_kernel<PIXT, 8, SECV, false, SELV>), dim3(grid * 8), dim3(64), 0, stream, R, (const PIXT *)rec, (PIXT *)fin, blk, nullptr, nullptr);  \
    else if (sse_here) hipLaunchKernelGGL((cdef_sb_kernel<PIXT, 1, SECV, true, SELV>), dim3(grid), dim3(64), 0, stream, R, (const PIXT *)rec, (PIXT *)fin, blk, (const PIXT *)src, sse);  \
    else hipLaunchKernelGGL((cdef_sb_kernel<PIXT, 1, SECV, false, SELV>), dim3(grid), dim3(64), 0, stream, R, (const PIXT *)rec, (PIXT *)fin, blk, nullptr, nullptr);  \
  } while (0)
#define CDEF_LAUNCH(PIXT) do { if (sel) CDEF_LAUNCH2(PIXT, true, true); else if (sec) CDEF_LAUNCH2(PIXT, true, false); else CDEF_LAUNCH2(PIXT, false, false); } while (0)
  if (R.bit_depth == 8) CDEF_LAUNCH(uint8_t); else CDEF_LAUNCH(uint16_t);
#undef CDEF_LAUNCH2
#undef CDEF_LAUNCH
  return hipGetLastError();
}

extern "C" hipError_t av1mi_launch_cdef_search(const Av1miDevParams *P, const void *rec, const void *src, const Av1miBlkInfo *blk, uint8_t *hdr_blob,
                                               int frame0, int count, hipStream_t stream) {
  if (!P->cdef_search || !P->cdef_err || !P->cdef_idx || !P->cdef_sel) return hipErrorInvalidValue;
  const int grid = count * P->sb_rows * P->sb_cols;
  const int ns = count == 1 ? 8 : 1;
#define CS_LAUNCH(PIXT, NSV) hipLaunchKernelGGL((cdef_search_kernel<PIXT, NSV>), dim3(grid * NSV), dim3(64), 0, stream, *P, frame0, (const PIXT *)rec, (const PIXT *)src, blk)
  if (P->bit_depth == 8) { if (ns == 8) CS_LAUNCH(uint8_t, 8); else CS_LAUNCH(uint8_t, 1); }
  else { if (ns == 8) CS_LAUNCH(uint16_t, 8); else CS_LAUNCH(uint16_t, 1); }
#undef CS_LAUNCH
  hipLaunchKernelGGL(cdef_select_kernel, dim3(count), dim3(512), 0, stream, *P, frame0, hdr_blob);
  return hipGetLastError();
}
