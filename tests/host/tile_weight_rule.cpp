// Host-side check of the rule weight -> class (av1-base_amd/csrc/tile_weight_rule.h), built as plain C++ by
// tests/test_sym_order_host.py: for every weight from 0 up to the largest sum of a tile of 2 x 2 superblocks the class lies in
// 0 .. 15 and never decreases; weight 0 - and nothing else - is class 0; the largest sum of a one-superblock tile and of a 2 x 2 tile
// are in the top class, and so is the bound the header names; the table a walk over the classes indexes holds 16 rows.
#include <cstdint>
#include <cstdio>

#include "../../av1-base_amd/csrc/tile_weight_rule.h"

int main() {
  const uint32_t max1 = AV1MI_TILE_WEIGHT_MAX_SB, max4 = 4 * AV1MI_TILE_WEIGHT_MAX_SB;
  static_assert(AV1MI_TILE_CLASSES == 16, "16 classes");
  static_assert(AV1MI_TILE_WEIGHT_MAX_SB == 4 * 1024 + 8 * 256, "four 32x32 luma and eight 16x16 chroma blocks");
  int prev = 0, seen[AV1MI_TILE_CLASSES] = {0};
  for (uint32_t w = 0; w <= max4; w++) {
    const int c = av1mi_tile_weight_class(w);
    if (c < 0 || c >= AV1MI_TILE_CLASSES) { printf("weight %u: class %d out of range\n", w, c); return 1; }
    if (c < prev) { printf("weight %u: class %d after %d\n", w, c, prev); return 1; }
    if ((c == 0) != (w == 0)) { printf("weight %u: class %d\n", w, c); return 1; }
    if ((c == AV1MI_TILE_CLASSES - 1) != (w >= (uint32_t)AV1MI_TILE_WEIGHT_TOP)) { printf("weight %u: class %d against the top bound\n", w, c); return 1; }
    seen[c]++;
    prev = c;
  }
  if (av1mi_tile_weight_class(0) != 0) return 1;
  if (av1mi_tile_weight_class(max1) != AV1MI_TILE_CLASSES - 1 || av1mi_tile_weight_class(max4) != AV1MI_TILE_CLASSES - 1) return 1;
  if (av1mi_tile_weight_class(UINT32_MAX) != AV1MI_TILE_CLASSES - 1) return 1;   // (no wrap at the far end either)
  if ((uint32_t)AV1MI_TILE_WEIGHT_TOP > max1) { printf("the top class starts beyond a one-superblock tile's largest sum\n"); return 1; }
  for (int c = 0; c < AV1MI_TILE_CLASSES; c++) if (!seen[c]) { printf("class %d is never used\n", c); return 1; }
  printf("ok %d %u\n", AV1MI_TILE_CLASSES, (unsigned)AV1MI_TILE_WEIGHT_TOP);
  return 0;
}
