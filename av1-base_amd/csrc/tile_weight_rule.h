// tile_weight_rule.h - the order symbolize takes a key-frame chunk's tiles in, for host and device.
//
// A tile's WEIGHT is the sum of the eobs of the transform blocks its reconstruction wave coded: the number of coefficient positions
// symbolize will walk, known one kernel before symbolize runs.  The weight picks one of 16 CLASSES; symbolize takes the classes from
// the heaviest down, so that the long tiles start while the chip is full and the launch ends on short ones.  Non-normative: every tile
// writes only its own slots, the order changes no byte.
//
//   class 0        weight 0 (every block of the tile skipped), and nothing else
//   class k, 1..14 weights 128 (k - 1) + 1 .. 128 k
//   class 15       weights above 1792
//
// The step: what matters is the END of the queue - the tiles that start when the queue is empty should be the lightest, and the ones
// that start with the launch all start at once whatever their order - so the classes resolve the bulk of the weights and the heaviest
// tiles share the top class.  Measured on the 30 600 tiles of a 1080p x 60 chunk at CQ 30: classes 1 .. 14 hold 190,
// 1 191, 1 628 and then 1 300 - 2 330 tiles each, class 0 none, the top class 4 939 - about the 5 290 waves of symbolize that are
// resident at once, i.e. the first batch.  The largest weights - 6 144 for a tile of one superblock (4 x 1024 + 8 x 256), four times
// that for one of 2 x 2 - land in the top class; no weight can wrap the rule.
#ifndef AV1MI_TILE_WEIGHT_RULE_H
#define AV1MI_TILE_WEIGHT_RULE_H
#include <stdint.h>
#ifdef __HIPCC__
#define AV1MI_TW_HD __host__ __device__
#else
#define AV1MI_TW_HD
#endif

#define AV1MI_TILE_CLASSES 16
#define AV1MI_TILE_WEIGHT_STEP_LOG2 7
#define AV1MI_TILE_WEIGHT_TOP (((AV1MI_TILE_CLASSES - 2) << AV1MI_TILE_WEIGHT_STEP_LOG2) + 1)   /* the smallest weight of the top class */
#define AV1MI_TILE_WEIGHT_MAX_SB 6144   /* 4:2:0 superblock: 4096 luma + 2 x 1024 chroma coefficient positions */

AV1MI_TW_HD inline int av1mi_tile_weight_class(uint32_t weight) {
  if (weight >= (uint32_t)AV1MI_TILE_WEIGHT_TOP) return AV1MI_TILE_CLASSES - 1;   // (before the rounding: no sum can wrap)
  return (int)((weight + (1u << AV1MI_TILE_WEIGHT_STEP_LOG2) - 1u) >> AV1MI_TILE_WEIGHT_STEP_LOG2);
}

#endif
