// me_rule.h - the rules of the motion search that more than one place applies, compiled for the
// device and for the host: which candidates a block may take, what a candidate costs, how the search's keys are laid out and how the
// reconstruction reads a leaf's motion from them.  The kernels of me_kernel.hip and the two key reads of recon_kernel.hip go through these;
// tests/host/me_rule_host.cpp runs them on the CPU against the restatement in tests/part_inter_ref.py.
#ifndef AV1MI_ME_RULE_H
#define AV1MI_ME_RULE_H
#include <stdint.h>

#ifdef __HIPCC__
#define AV1MI_ME_INLINE __host__ __device__ __forceinline__
#else
#define AV1MI_ME_INLINE inline
#endif

AV1MI_ME_INLINE int av1mi_me_iabs(int v) { return v < 0 ? -v : v; }

// ---- reach: a displaced block stays within AV1MI_ME_MARGIN samples of the frame.  One axis at a time - a wave tests y once and x per
// lane: the block [p, p + n) displaced by d whole samples, on an axis of `size` samples ...
#define AV1MI_ME_MARGIN 16
AV1MI_ME_INLINE bool av1mi_me_reach(int p, int d, int n, int size) { return p + d >= -AV1MI_ME_MARGIN && p + d + n <= size + AV1MI_ME_MARGIN; }
// ... and displaced by m eighth samples (the sub-sample refinement), asked the other way round: is it out of reach?
AV1MI_ME_INLINE bool av1mi_me_out_of_reach8(int p, int m, int n, int size) {
  return p * 8 + m < -AV1MI_ME_MARGIN * 8 || (p + n) * 8 + m > (size + AV1MI_ME_MARGIN) * 8;
}
// The pre-search moves a whole superblock: its extent on an axis is clipped to the frame (the superblock at p of an axis of `size` samples)
AV1MI_ME_INLINE int av1mi_me_sb_extent(int p, int size) { return size - p < 64 ? size - p : 64; }

// ---- the centre code: the centre (Cx, Cy) of a superblock's search window in units of 8 luma samples, 12-bit two's complement each,
// (Cy / 8 & 0xFFF) << 12 | (Cx / 8 & 0xFFF) - zero without the quarter-resolution pre-search (av1mi_params.me_presearch).
AV1MI_ME_INLINE int av1mi_sext12(uint32_t v) { return (int)((v & 0xFFFu) ^ 0x800u) - 0x800; }
AV1MI_ME_INLINE void av1mi_me_centre_decode(uint32_t code, int *ccx, int *ccy) { *ccx = 8 * av1mi_sext12(code); *ccy = 8 * av1mi_sext12(code >> 12); }
// The pre-search's displacement dq (quarter-resolution samples: 4 luma samples) as a centre in luma samples: rounded to units of 8
AV1MI_ME_INLINE int av1mi_me_centre_of_quarter(int dq) { return ((dq + 1) >> 1) * 8; }
AV1MI_ME_INLINE uint32_t av1mi_me_centre_encode(int dqx, int dqy) {
  return ((uint32_t)((av1mi_me_centre_of_quarter(dqy) >> 3) & 0xFFF) << 12) | (uint32_t)((av1mi_me_centre_of_quarter(dqx) >> 3) & 0xFFF);
}

// ---- the integer search.  Candidate (dyi, dxi), 0 <= dyi, dxi <= 2 R, is the vector (dx, dy) = (dxi - R + Cx, dyi - R + Cy); its cost for a
// block of n x n is SAD + n (|dx| + |dy|) < 2^24 and its index dyi (2 R + 1) + dxi - raster order, so that a minimum over keys that hold
// (cost, index) breaks ties to the first candidate.
AV1MI_ME_INLINE uint32_t av1mi_me_cost(uint32_t sad, int n, int dx, int dy) { return sad + (uint32_t)n * (uint32_t)(av1mi_me_iabs(dx) + av1mi_me_iabs(dy)); }
AV1MI_ME_INLINE uint32_t av1mi_me_index(int dyi, int dxi, int R) { return (uint32_t)(dyi * (2 * R + 1) + dxi); }

// The leaf key (me_kernel.hip -> recon_kernel.hip): per leaf, at its origin's 8x8 unit, the minimum over its candidates of
//   (centre code << 40) | (cost << 16) | index
// - the code is the same for every candidate of a leaf, so the minimum is taken over (cost, index); all-ones: no candidate was valid.
#define AV1MI_ME_KEY_NONE (~0ull)
AV1MI_ME_INLINE unsigned long long av1mi_me_key(uint32_t centre_code, uint32_t cost, uint32_t index) {
  return ((unsigned long long)centre_code << 40) | ((unsigned long long)cost << 16) | (unsigned long long)index;
}
AV1MI_ME_INLINE uint32_t av1mi_me_key_cost(unsigned long long key) { return (uint32_t)((key >> 16) & 0xFFFFFF); }
AV1MI_ME_INLINE uint32_t av1mi_me_key_index(unsigned long long key) { return (uint32_t)(key & 0xFFFF); }
AV1MI_ME_INLINE void av1mi_me_key_decode(unsigned long long key, int R, int *dy, int *dx, int *cost) {
  const int nc = 2 * R + 1, idx = (int)av1mi_me_key_index(key);
  int ccx, ccy;
  av1mi_me_centre_decode((uint32_t)(key >> 40), &ccx, &ccy);
  *dy = idx / nc - R + ccy;
  *dx = idx % nc - R + ccx;
  *cost = (int)av1mi_me_key_cost(key);
}

// The node key (node mode: the search's node tables, part_inter_rule.h; and the pre-search's own minimum): 32 bits, (cost << 11) | index,
// cost < 2^21 (nodes up to 32x32), index < 2^11 (R <= 16: 33 x 33 candidates); all-ones: no candidate was valid.
#define AV1MI_ME_NODE_INDEX_BITS 11
#define AV1MI_ME_NODE_NONE 0xFFFFFFFFu
AV1MI_ME_INLINE uint32_t av1mi_me_node_key(uint32_t cost, uint32_t index) { return (cost << AV1MI_ME_NODE_INDEX_BITS) | index; }
AV1MI_ME_INLINE uint32_t av1mi_me_node_cost(uint32_t key) { return key >> AV1MI_ME_NODE_INDEX_BITS; }
AV1MI_ME_INLINE uint32_t av1mi_me_node_index(uint32_t key) { return key & ((1u << AV1MI_ME_NODE_INDEX_BITS) - 1); }

// ---- the sub-sample refinement (subpel = 1).  Stage `step` = 8: the integer winner itself, re-costed; 4, then 2: the eight neighbours of
// the stage's base vector at that distance in eighth samples, k = 0 .. 8 in (row, col) raster order, the centre k = 4 skipped.
// Is k a candidate of the stage, and which vector is it?  (The kernel calls the three pieces: through the one function with the vector
// behind pointers subpel_refine_kernel ran 1 % longer)
AV1MI_ME_INLINE bool av1mi_me_refine_is_cand(int step, int k) { return (k == 4) == (step == 8); }
AV1MI_ME_INLINE int av1mi_me_refine_row(int step, int k, int base_row) { return base_row + (step == 8 ? 0 : (k / 3 - 1) * step); }
AV1MI_ME_INLINE int av1mi_me_refine_col(int step, int k, int base_col) { return base_col + (step == 8 ? 0 : (k % 3 - 1) * step); }
AV1MI_ME_INLINE bool av1mi_me_refine_cand(int step, int k, int base_row, int base_col, int *mr, int *mc) {
  *mr = av1mi_me_refine_row(step, k, base_row);
  *mc = av1mi_me_refine_col(step, k, base_col);
  return av1mi_me_refine_is_cand(step, k);
}
// Its cost from the SATD of the n x n block (the sum of the absolute 8x8 Hadamard coefficients, not yet >> 3); a candidate replaces the
// stage's best only when strictly cheaper
AV1MI_ME_INLINE long av1mi_me_refine_cost(int satd, int n, int mr, int mc) {
  return (long)(satd >> 3) + (((long)n * (av1mi_me_iabs(mr) + av1mi_me_iabs(mc))) >> 3);
}
// The refined key, per leaf: (SAD << 36) | (u16 mv.row << 16) | u16 mv.col, the vector in eighth samples
AV1MI_ME_INLINE unsigned long long av1mi_me_refined_key(int sad, int mv_row, int mv_col) {
  return ((unsigned long long)(uint32_t)sad << 36) | ((unsigned long long)(uint16_t)(int16_t)mv_row << 16) | (uint16_t)(int16_t)mv_col;
}

// ---- what the reconstruction reads of a leaf of n x n: the vector in eighth samples and the luma SAD at that vector - from the refined key
// with subpel, otherwise from the leaf key, whose cost holds the vector's penalty
AV1MI_ME_INLINE void av1mi_me_leaf_motion(unsigned long long key, int subpel, int R, int n, int *mv_row, int *mv_col, int *sad) {
  if (subpel) {
    *mv_row = (int16_t)(key >> 16); *mv_col = (int16_t)key;
    *sad = (int)(key >> 36);
  } else {
    int dy, dx, cost;
    av1mi_me_key_decode(key, R, &dy, &dx, &cost);
    *mv_row = dy * 8; *mv_col = dx * 8;
    *sad = cost - n * (av1mi_me_iabs(dx) + av1mi_me_iabs(dy));
  }
}
#endif
