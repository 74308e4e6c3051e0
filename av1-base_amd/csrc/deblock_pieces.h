// deblock_pieces.h - the pieces of the deblocking filter (spec §7.14) that more than one place needs, compiled for the device and for
// the host: the sample filter, the edge predicate, the level's limits, the level search's candidate pool and first-minimum rule
//  and the geometry of the search's superblock tile.  deblock_kernel and deblock_search_kernel
// (deblock_kernel.hip) both filter through these, so the search scores exactly what the filter will do; tests/host/deblock_pieces_host.cpp
// runs them on the CPU against oracle/av1o_deblock.c.
#ifndef AV1MI_DEBLOCK_PIECES_H
#define AV1MI_DEBLOCK_PIECES_H
#include "av1mi_dev.h"

#ifdef __HIPCC__
#define AV1MI_LF_INLINE __host__ __device__ __forceinline__
#else
#define AV1MI_LF_INLINE inline
#endif

AV1MI_LF_INLINE int av1mi_lf_iabs(int v) { return v < 0 ? -v : v; }
AV1MI_LF_INLINE int av1mi_lf_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one sample position across an edge: px[-k*step] = p(k-1), px[k*step] = q(k).  len: 4, 6 (chroma), 8 or 16 = filterLen
template <typename PIX, typename STEP>
AV1MI_LF_INLINE void av1mi_lf_filter_sample(PIX *px, STEP step, int plane, int lim, int blim, int thr, int len, int bd) {
  const int one = 1 << (bd - 8);
  int t[16];  // t[8 + i] = sample i (i < 0: p(-i-1), i >= 0: q(i)) for i in -8..7
  const int reach = len == 16 ? 7 : (len == 8 ? 4 : (len == 6 ? 3 : 2));
#pragma unroll
  for (int i = -7; i < 7; i++) t[8 + i] = (i >= -reach && i < reach) ? (int)px[i * step] : 0;
#define AV1MI_LF_P(k) t[7 - (k)]
#define AV1MI_LF_Q(k) t[8 + (k)]
  const int p0 = AV1MI_LF_P(0), p1 = AV1MI_LF_P(1), q0 = AV1MI_LF_Q(0), q1 = AV1MI_LF_Q(1);
  const bool hev = av1mi_lf_iabs(p1 - p0) > thr || av1mi_lf_iabs(q1 - q0) > thr;
  bool mask = av1mi_lf_iabs(p1 - p0) > lim || av1mi_lf_iabs(q1 - q0) > lim || av1mi_lf_iabs(p0 - q0) * 2 + av1mi_lf_iabs(p1 - q1) / 2 > blim;
  if (len >= 6) mask = mask || av1mi_lf_iabs(AV1MI_LF_P(2) - p1) > lim || av1mi_lf_iabs(AV1MI_LF_Q(2) - q1) > lim;
  if (len >= 8) mask = mask || av1mi_lf_iabs(AV1MI_LF_P(3) - AV1MI_LF_P(2)) > lim || av1mi_lf_iabs(AV1MI_LF_Q(3) - AV1MI_LF_Q(2)) > lim;
  if (mask) return;
  bool flat = false, flat2 = false;
  if (len >= 6) {
    flat = av1mi_lf_iabs(p1 - p0) <= one && av1mi_lf_iabs(q1 - q0) <= one && av1mi_lf_iabs(AV1MI_LF_P(2) - p0) <= one && av1mi_lf_iabs(AV1MI_LF_Q(2) - q0) <= one;
    if (len >= 8) flat = flat && av1mi_lf_iabs(AV1MI_LF_P(3) - p0) <= one && av1mi_lf_iabs(AV1MI_LF_Q(3) - q0) <= one;
  }
  if (len >= 16) flat2 = av1mi_lf_iabs(AV1MI_LF_P(4) - p0) <= one && av1mi_lf_iabs(AV1MI_LF_Q(4) - q0) <= one && av1mi_lf_iabs(AV1MI_LF_P(5) - p0) <= one &&
                         av1mi_lf_iabs(AV1MI_LF_Q(5) - q0) <= one && av1mi_lf_iabs(AV1MI_LF_P(6) - p0) <= one && av1mi_lf_iabs(AV1MI_LF_Q(6) - q0) <= one;
  if (len == 4 || !flat) {
    // narrow filter §7.14.6.3
    const int lo = -(1 << (bd - 1)), hi = (1 << (bd - 1)) - 1, half = 0x80 << (bd - 8);
    const int ps1 = p1 - half, ps0 = p0 - half, qs0 = q0 - half, qs1 = q1 - half;
    int f = hev ? av1mi_lf_clampi(ps1 - qs1, lo, hi) : 0;
    f = av1mi_lf_clampi(f + 3 * (qs0 - ps0), lo, hi);
    const int f1 = av1mi_lf_clampi(f + 4, lo, hi) >> 3, f2 = av1mi_lf_clampi(f + 3, lo, hi) >> 3;
    px[0] = (PIX)(av1mi_lf_clampi(qs0 - f1, lo, hi) + half);
    px[-step] = (PIX)(av1mi_lf_clampi(ps0 + f2, lo, hi) + half);
    if (!hev) {
      const int g = (f1 + 1) >> 1;
      px[step] = (PIX)(av1mi_lf_clampi(qs1 - g, lo, hi) + half);
      px[-2 * step] = (PIX)(av1mi_lf_clampi(ps1 + g, lo, hi) + half);
    }
  } else {
    // wide filter §7.14.6.4: 2n + 1 taps (n = 6 / 3 / 2) whose weights sum to 1 << log2size
    const int log2size = (len == 16 && flat2) ? 4 : 3;
    const int n = log2size == 4 ? 6 : (plane == 0 ? 3 : 2), n2 = (log2size == 3 && plane == 0) ? 0 : 1;
    int out[12];
#pragma unroll
    for (int i = -6; i < 6; i++) {
      int s = 0;
      if (i >= -n && i < n) {
#pragma unroll
        for (int j = -6; j <= 6; j++) {
          if (j < -n || j > n) continue;
          const int p = av1mi_lf_clampi(i + j, -(n + 1), n);
          s += t[8 + p] * (av1mi_lf_iabs(j) <= n2 ? 2 : 1);
        }
        s = (s + (1 << (log2size - 1))) >> log2size;
      }
      out[i + 6] = s;
    }
#pragma unroll
    for (int i = -6; i < 6; i++)
      if (i >= -n && i < n) px[i * step] = (PIX)out[i + 6];
  }
#undef AV1MI_LF_P
#undef AV1MI_LF_Q
}

// The edge predicate (§7.14.2, §7.14.3 for this build: square blocks, transform == block).  (r4, c4): a 4x4 position of the plane;
// pass 0: the vertical edge on its left, 1: the horizontal edge above it.  info: the frame's block info (8x8 luma units, b8_cols per
// row).  The filter length 4 / 6 / 8 / 16, or 0: no edge is filtered there (off screen - beyond the signalled size -, the frame's
// first column / row, or not a block edge).  A position outside the frame is off screen: nothing is read for it.
AV1MI_LF_INLINE int av1mi_lf_edge_len(int plane, int pass, int r4, int c4, const Av1miBlkInfo *info, int b8_cols, int true_w, int true_h) {
  const int ss = plane > 0;
  const int row = r4 << ss, col = c4 << ss;                          // the same in luma 4x4 units
  if (r4 < 0 || c4 < 0 || col * 4 >= true_w || row * 4 >= true_h) return 0;   // onScreen (§7.14.2)
  if (pass == 0 ? c4 == 0 : r4 == 0) return 0;
  const int prow = row - (pass ? 1 << ss : 0), pcol = col - (pass ? 0 : 1 << ss);
  const int bsl = info[(size_t)(row >> 1) * b8_cols + (col >> 1)].bsl, pbsl = info[(size_t)(prow >> 1) * b8_cols + (pcol >> 1)].bsl;
  int txw = (1 << bsl) >> ss, ptxw = (1 << pbsl) >> ss;
  txw = txw < 4 ? 4 : txw; ptxw = ptxw < 4 ? 4 : ptxw;
  if ((((pass == 0 ? c4 : r4) * 4) & (txw - 1)) != 0) return 0;      // not a transform (= block) edge
  const int base = txw < ptxw ? txw : ptxw;
  return plane == 0 ? (base >= 16 ? 16 : base) : (base >= 8 ? 6 : 4);
}

// §7.14.4: the limits of a level at the samples' scale
AV1MI_LF_INLINE void av1mi_lf_limits(int lvl, int sharp, int bit_depth, int *lim, int *blim, int *thr) {
  const int shift = sharp > 4 ? 2 : (sharp > 0 ? 1 : 0);
  const int limit = sharp > 0 ? av1mi_lf_clampi(lvl >> shift, 1, 9 - sharp) : ((lvl >> shift) > 1 ? (lvl >> shift) : 1);
  const int sh = bit_depth - 8;
  *lim = limit << sh; *blim = (2 * (lvl + 2) + limit) << sh; *thr = (lvl >> 4) << sh;
}

// ---- the level search (av1mi_params.deblock = 2).  g: the level the quantiser formula gives the frame kind.
// Candidate i of a plane is clamp(g + D[i], 1 (luma) / 0 (chroma), 63); the plane takes the FIRST i that minimises its squared error.
#define AV1MI_LF_CANDS 16
AV1MI_LF_INLINE int av1mi_lf_delta(int i) {
  return i < 8 ? (i < 4 ? (i < 2 ? (i ? -8 : -12) : (i == 2 ? -6 : -4)) : i - 7) : (i < 12 ? i - 7 : (i < 14 ? (i == 12 ? 6 : 8) : (i == 14 ? 12 : 16)));
}
AV1MI_LF_INLINE int av1mi_lf_pool(int g, int i, int chroma) { return av1mi_lf_clampi(g + av1mi_lf_delta(i), chroma ? 0 : 1, 63); }
AV1MI_LF_INLINE int av1mi_lf_first_min(const unsigned long long *e) {
  int b = 0;
  for (int i = 1; i < AV1MI_LF_CANDS; i++) if (e[i] < e[b]) b = i;
  return b;
}

// ---- the search's tile: one 64x64 superblock of one plane (32x32 in chroma) with a halo of 8 luma / 4 chroma samples all round, in
// 16-bit samples at a row pitch of AV1MI_LF_PITCH (odd in 32-bit words: the lanes of the vertical pass, one tile row each, hit
// different LDS banks).  A filter reads at most 7 / 3 samples on each side of an edge and modifies at most 6 / 2, and within a pass no edge
// reads what another writes, so the interior after both passes needs: the horizontal edges at interior rows 0, U, .. S (U = 8 / 4, the
// smallest block) on the interior's columns, over rows -7 .. S + 6 of the vertically filtered tile; and for those the vertical edges at
// interior columns 0, U, .. S on every tile row, over columns -7 .. S + 6 of the unfiltered tile.
#define AV1MI_LF_PITCH 82
#define AV1MI_LF_TILE_SAMPLES (80 * AV1MI_LF_PITCH)
#define AV1MI_LF_EDGES 9      // S / U + 1, luma and chroma alike
#define AV1MI_LF_SEGS 20      // 4-sample segments along an edge: (S + 2 H) / 4 in luma
struct Av1miLfTile {
  int plane, S, H, U, T;      // interior size, halo, edge pitch, tile size S + 2 H
  int x0, y0;                 // the interior's origin in the plane
  int pw, ph;                 // the plane's coded size
};
AV1MI_LF_INLINE Av1miLfTile av1mi_lf_tile(int plane, int sbr, int sbc, int width, int height) {
  Av1miLfTile t;
  const int ss = plane > 0;
  t.plane = plane; t.S = 64 >> ss; t.H = 8 >> ss; t.U = 8 >> ss; t.T = t.S + 2 * t.H;
  t.x0 = sbc * t.S; t.y0 = sbr * t.S; t.pw = width >> ss; t.ph = height >> ss;
  return t;
}
// where tile sample (ty, tx) is loaded from: the plane position, clamped into the plane (a clamped sample stands for a position that
// does not exist; no filtered edge reaches one)
AV1MI_LF_INLINE void av1mi_lf_tile_source(const Av1miLfTile &t, int ty, int tx, int *py, int *px) {
  *py = av1mi_lf_clampi(t.y0 - t.H + ty, 0, t.ph - 1); *px = av1mi_lf_clampi(t.x0 - t.H + tx, 0, t.pw - 1);
}
// lines of a pass: pass 0 - AV1MI_LF_EDGES * T (edge e, tile row j), pass 1 - AV1MI_LF_EDGES * S (edge e, interior column j)
AV1MI_LF_INLINE int av1mi_lf_tile_lines(const Av1miLfTile &t, int pass) { return AV1MI_LF_EDGES * (pass ? t.S : t.T); }
// filter length of segment k (lines 4 k .. 4 k + 3) of edge e of a pass, 0 = none: the edge predicate at the segment's plane position
AV1MI_LF_INLINE int av1mi_lf_tile_seg_len(const Av1miLfTile &t, int pass, int e, int k, const Av1miBlkInfo *info, int b8_cols, int true_w, int true_h) {
  const int px = pass ? t.x0 + 4 * k : t.x0 + e * t.U, py = pass ? t.y0 + e * t.U : t.y0 - t.H + 4 * k;
  if (px < 0 || py < 0 || px >= t.pw || py >= t.ph) return 0;
  return av1mi_lf_edge_len(t.plane, pass, py >> 2, px >> 2, info, b8_cols, true_w, true_h);
}
// line L of a pass: its edge and segment, and the tile offset of its q0 sample (the filter steps by 1 in pass 0, by the pitch in pass 1)
AV1MI_LF_INLINE int av1mi_lf_tile_line(const Av1miLfTile &t, int pass, int L, int *e, int *k) {
  const int n = pass ? t.S : t.T, j = L % n;
  *e = L / n; *k = j >> 2;
  return pass ? (t.H + *e * t.U) * AV1MI_LF_PITCH + t.H + j : j * AV1MI_LF_PITCH + t.H + *e * t.U;
}

#endif
