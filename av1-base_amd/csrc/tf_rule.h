// tf_rule.h - the rules of the key frames' temporal filter that more than one place applies, compiled for
// the device and for the host: how the switch packs into av1mi_params.me_presearch, how many followers a key frame has, the weight of a
// follower's sample from its errors, the blend, and the chroma predictor's taps at a luma vector.  The kernels of tf_kernel.hip and
// the host code (av1mi_syntax.cpp, av1mi_host.cpp) go through these; tests/host/tf_rule_host.cpp runs them on the CPU against the restatement in tests/tf_ref.py.
// The search's own rules - reach, cost, index, the node key - are me_rule.h's, with blocks of AV1MI_TF_BLOCK and a zero centre.
#ifndef AV1MI_TF_RULE_H
#define AV1MI_TF_RULE_H
#include <stdint.h>
#include "me_rule.h"

#define AV1MI_TF_BLOCK 16        // luma block of the search and of the weights; chroma: half of it
#define AV1MI_TF_MAX_FRAMES 7
#define AV1MI_TF_MAX_STRENGTH 7

// ---- the field: av1mi_params.me_presearch bit 0 = the pre-search, bits 8-10 = N followers, bits 12-14 = strength s; nothing else, and
// no strength without followers.  (include/av1mi.h has the same layout as macros for callers.)
AV1MI_ME_INLINE int av1mi_tf_field_presearch(uint32_t v) { return (int)(v & 1u); }
AV1MI_ME_INLINE int av1mi_tf_field_frames(uint32_t v) { return (int)((v >> 8) & 7u); }
AV1MI_ME_INLINE int av1mi_tf_field_strength(uint32_t v) { return (int)((v >> 12) & 7u); }
AV1MI_ME_INLINE bool av1mi_tf_field_ok(uint32_t v) { return !(v & ~0x7701u) && !(av1mi_tf_field_strength(v) && !av1mi_tf_field_frames(v)); }

// ---- the followers of key frame f (f % keyint == 0) of a chunk of n_frames: n = min(N, keyint - 1, n_frames - 1 - f)
AV1MI_ME_INLINE int av1mi_tf_followers(int N, int keyint, int n_frames, int f) {
  int n = N < keyint - 1 ? N : keyint - 1;
  n = n < n_frames - 1 - f ? n : n_frames - 1 - f;
  return n < 0 ? 0 : n;
}
// the key frames of a chunk, and the 16x16 blocks of a coded frame of w x h (raster order)
AV1MI_ME_INLINE int av1mi_tf_key_frames(int keyint, int n_frames) { return (n_frames + keyint - 1) / keyint; }
AV1MI_ME_INLINE int av1mi_tf_blocks(int size) { return (size + AV1MI_TF_BLOCK - 1) / AV1MI_TF_BLOCK; }

// ---- the weight of a follower's sample.  e = key - prediction; S = the sum of e^2 over the 3x3 window around the sample, positions
// clamped to the block (<= 9 * 1023^2 < 2^24); B = the sum of e^2 over the block of `samples` = 256 (luma) or 64 (chroma) samples
// (<= 256 * 1023^2 < 2^28; 9 B needs all 32 bits, unsigned).  sh = 3 + s + 2 (bd - 8); the index is
// min(15, (S >> sh) + ((9 B) >> (sh + log2 samples))) - the window's error plus the block's mean error at the same scale.
AV1MI_ME_INLINE int av1mi_tf_shift(int strength, int bit_depth) { return 3 + strength + 2 * (bit_depth - 8); }
AV1MI_ME_INLINE int av1mi_tf_index(uint32_t S, uint32_t B, int sh, int chroma) {
  const uint32_t i = (S >> sh) + ((9u * B) >> (sh + (chroma ? 6 : 8)));
  return (int)(i < 15u ? i : 15u);
}
AV1MI_ME_INLINE int av1mi_tf_weight(int index) {
  // { 16, 12, 10, 8, 6, 5, 4, 3, 2, 2, 1, 1, 1, 1, 0, 0 }[index]: entries 1 .. 15 as the nibbles of one constant (an array indexed per
  // sample would live in the kernel's scratch memory)
  return index == 0 ? 16 : (int)((0x0011112234568AC0ull >> (4 * index)) & 15u);
}

// ---- the blend of a sample: the key weighs 16, follower t weighs w_t; num = 16 key + sum w_t pred_t, den = 16 + sum w_t (16 .. 128)
AV1MI_ME_INLINE int av1mi_tf_blend(uint32_t num, uint32_t den) { return (int)((num + den / 2) / den); }

// ---- the chroma prediction at the luma vector (dx, dy): the chroma vector is (dx >> 1, dy >> 1), arithmetic shifts, and an odd
// component averages two neighbours.  a = the sample at the base, b = right of it, c = below, d = below right (coordinates clamped by the caller)
AV1MI_ME_INLINE int av1mi_tf_chroma_base(int p, int d) { return p + (d >> 1); }
AV1MI_ME_INLINE int av1mi_tf_chroma_pred(int a, int b, int c, int d, int dx, int dy) {
  const int ox = dx & 1, oy = dy & 1;
  if (ox && oy) return (a + b + c + d + 2) >> 2;
  if (ox) return (a + b + 1) >> 1;
  if (oy) return (a + c + 1) >> 1;
  return a;
}
#endif
