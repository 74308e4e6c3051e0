// tf_search.h - the whole-sample full search of one 16x16 luma block between two SOURCE frames, on one wave: the body that
// tf_search_kernel (tf_kernel.hip: a key frame against a follower) and tpl_cost_kernel (tpl_kernel.hip: a frame against the frame before
// it) share.  +-R whole samples around zero with me_rule.h's reach, cost, index and node key - the scheme of motion_search_kernel
// (packed sample pairs, v_sad_u16, DPP row rotations as operands of the additions) laid out for one block: lane = (row of the block,
// one of four dy) so that a pass over the 2R+1 dx covers four dy, the 16 lanes of a DPP row are the block's 16 rows, and the row's sum is
// the candidate's SAD.  Interior blocks load their rows in whole words (with one-sample loads everywhere the filter's launch took 4.7
// times as long: DESIGN.md §5l).  Device code only.
#ifndef AV1MI_TF_SEARCH_H
#define AV1MI_TF_SEARCH_H
#include <hip/hip_runtime.h>
#include "tf_rule.h"

__device__ __forceinline__ int tf_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// sum over the 16 lanes of a DPP row, in every lane of the row: rotations within the row as operands of the additions
__device__ __forceinline__ uint32_t tf_row_sum_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);   // row_ror 8, 4, 2, 1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);
  return v;
}
// minimum over the wave, wave-uniform: over each row with rotations, then one v_readlane per row
__device__ __forceinline__ uint32_t tf_wave_min_u32(uint32_t v) {
  uint32_t t;
  t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x128, 0xF, 0xF, false); v = t < v ? t : v;
  t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x124, 0xF, 0xF, false); v = t < v ? t : v;
  t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x122, 0xF, 0xF, false); v = t < v ? t : v;
  t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x121, 0xF, 0xF, false); v = t < v ? t : v;
  uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
  t = (uint32_t)__builtin_amdgcn_readlane((int)v, 16); m = t < m ? t : m;
  t = (uint32_t)__builtin_amdgcn_readlane((int)v, 32); m = t < m ? t : m;
  t = (uint32_t)__builtin_amdgcn_readlane((int)v, 48); m = t < m ? t : m;
  return m;
}

// 2 NP consecutive samples of a row from x0 on, two per register: pair[i] = samples (x0 + 2i, x0 + 2i + 1).  `inside`: all of them lie
// in the row and x0 is a multiple of 8 samples (8 bytes for 8-bit samples, 16 for 16-bit ones: the loads are that wide; NP is a
// multiple of 4) - else one sample at a time with clamped coordinates.
template <typename PIX, int NP>
__device__ __forceinline__ void tf_load_pairs(const PIX *__restrict__ row, int x0, int W, bool inside, uint32_t *pair) {
  static_assert(NP % 4 == 0, "whole 8-sample loads");
  if (inside) {
    if constexpr (sizeof(PIX) == 2) {
      const uint4 *v = reinterpret_cast<const uint4 *>(row + x0);
#pragma unroll
      for (int j = 0; j < NP / 4; j++) { const uint4 d = v[j]; pair[4 * j] = d.x; pair[4 * j + 1] = d.y; pair[4 * j + 2] = d.z; pair[4 * j + 3] = d.w; }
    } else {
      const uint2 *v = reinterpret_cast<const uint2 *>(row + x0);
#pragma unroll
      for (int j = 0; j < NP / 4; j++) {
        const uint2 d = v[j];
        pair[4 * j] = (d.x & 0xFFu) | ((d.x << 8) & 0xFF0000u); pair[4 * j + 1] = ((d.x >> 16) & 0xFFu) | ((d.x >> 8) & 0xFF0000u);
        pair[4 * j + 2] = (d.y & 0xFFu) | ((d.y << 8) & 0xFF0000u); pair[4 * j + 3] = ((d.y >> 16) & 0xFFu) | ((d.y >> 8) & 0xFF0000u);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NP; i++) pair[i] = (uint32_t)row[tf_clampi(x0 + 2 * i, W - 1)] | ((uint32_t)row[tf_clampi(x0 + 2 * i + 1, W - 1)] << 16);
  }
}

// Row (lane & 15) of the block at (x, y) of the luma plane `cur` (W x H samples, rows `stride` apart), coordinates clamped to the frame
// (an overhanging block), two samples per register.  (Interior blocks load whole words: the plane is 16-byte aligned, x is a multiple
// of 8, and so are the rows' strides.)
template <typename PIX>
__device__ __forceinline__ void tf_block_row(const PIX *__restrict__ cur, int x, int y, int W, int H, int stride, int lane, uint32_t (&s2)[8]) {
  tf_load_pairs<PIX, 8>(cur + (size_t)tf_clampi(y + (lane & 15), H - 1) * stride, x, W, x + AV1MI_TF_BLOCK <= W, s2);
}

// The search of the block at (x, y) of `cur` in `ref` (the luma planes of two frames of one layout, 16-byte aligned): returns the winner's
// node key, wave-uniform - (0, 0) is always within reach, never all-ones - and leaves the block's rows in s2 (tf_block_row).
template <typename PIX, int R>
__device__ __forceinline__ uint32_t tf_search_block(const PIX *__restrict__ cur, const PIX *__restrict__ ref, int x, int y, int W, int H, int stride,
                                                    int lane, uint32_t (&s2)[8]) {
  constexpr int NC = 2 * R + 1, PASSES = (NC + 3) / 4;
  static_assert(NC * NC <= (1 << AV1MI_ME_NODE_INDEX_BITS), "a node key holds an 11-bit candidate index");
  const int r = lane & 15, q = lane >> 4;
  // (interior blocks - the window of every candidate inside the row - load whole words: R is a multiple of 8)
  const bool in_ref = x - R >= 0 && x + AV1MI_TF_BLOCK + R <= W;
  tf_block_row<PIX>(cur, x, y, W, H, stride, lane, s2);
  // the dxi within reach of the frame, one bit each (wave-uniform; one mask instead of a flag per dxi kept across the passes)
  unsigned long long x_ok = 0;
  for (int dxi = 0; dxi < NC; dxi++) x_ok |= (unsigned long long)av1mi_me_reach(x, dxi - R, AV1MI_TF_BLOCK, W) << dxi;
  uint32_t best = AV1MI_ME_NODE_NONE;   // this lane's candidates: dx = its row position (mod 16), dy = 4 pass + q
  for (int pass = 0; pass < PASSES; pass++) {
    const int dyi = pass * 4 + q;
    const bool live = dyi < NC;
    const int dy = (live ? dyi : NC - 1) - R;
    // the reference's samples x - R .. x + 15 + R of row y + r + dy, coordinates clamped: rE[i] = samples (2i, 2i + 1), rO[i] = (2i + 1,
    // 2i + 2) - the block's pair i meets rE[i + dx / 2] for even dxi and rO[i + (dxi - 1) / 2] for odd
    uint32_t rE[8 + R], rO[8 + R];
    tf_load_pairs<PIX, 8 + R>(ref + (size_t)tf_clampi(y + r + dy, H - 1) * stride, x - R, W, in_ref, rE);
#pragma unroll
    for (int i = 0; i < 8 + R; i++) rO[i] = i < 8 + R - 1 ? (rE[i] >> 16) | (rE[i + 1] << 16) : 0u;
    const bool y_ok = live && av1mi_me_reach(y, dy, AV1MI_TF_BLOCK, H);
#pragma unroll
    for (int dxi = 0; dxi < NC; dxi++) {
      const int h = dxi >> 1;
      uint32_t a = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) a = __builtin_amdgcn_sad_u16(s2[i], (dxi & 1) ? rO[i + h] : rE[i + h], a);
      a = tf_row_sum_u32(a);   // over the block's 16 rows: the candidate's SAD, in every lane of the row
      const int dx = dxi - R;
      const bool ok = y_ok && r == (dxi & 15) && ((x_ok >> dxi) & 1);
      const uint32_t c = av1mi_me_node_key(av1mi_me_cost(a, AV1MI_TF_BLOCK, dx, dy), av1mi_me_index(dyi, dxi, R));
      best = ok && c < best ? c : best;
    }
  }
  return tf_wave_min_u32(best);
}

#endif
