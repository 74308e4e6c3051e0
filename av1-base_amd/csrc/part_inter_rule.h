// part_inter_rule.h - the partition of inter frames from the motion search's block costs (av1mi_params.partition_search = 2;
// DESIGN.md §3 item 2c).  One text for inter_partition_kernel (me_kernel.hip), the host program tests/host/part_inter_host.cpp and,
// restated in numpy, tests/part_inter_ref.py.
//
// Every node N of a superblock's partition tree - size n = 8 .. 64, origin inside the coded frame - has a leaf key L(N): the minimum
// over the candidates of the superblock's search window of (cost << 16) | index, cost = SAD + n (|dx| + |dy|), the displaced block
// within 16 samples of the frame, ties to the first candidate in raster order (applied to every node).  cL(N)
// is its cost field, AV1MI_PI_INF when no candidate is valid.  Bottom up, in the order of av1mi_node_split:
//   n = 8                                          J = cL
//   the frame edge forces a split                  J = sum of J(child) over the children whose origin is inside the frame
//   n <= 2^min_bs_log2                             J = cL
//   n >  2^max_bs_log2                             J = sum of J(child)
//   otherwise                                      S = sum of J(child) + T(n); the node splits iff S < cL (ties keep the larger block);
//                                                  J = min(S, cL)
// T(n) = (n n t) >> AV1MI_PI_K, t = ac_q(base_q_idx) >> 4: what four children gain over their parent by each picking its own minimum
// among near-equal candidates must not buy a split.  All sums fit 32 bits (J <= 4096 x 1023 + penalties < 2^23); a sum with an
// infinite term is infinite.
// The mask has av1mi_node_split's layout; a bit is set only for a node that was reached and decided: bits of forced nodes, of nodes
// under an unsplit node and of nodes outside the frame are 0.
#ifndef AV1MI_PART_INTER_RULE_H
#define AV1MI_PART_INTER_RULE_H
#include <stdint.h>
#include <stddef.h>
#ifndef AV1MI_HD
#ifdef __HIPCC__
#define AV1MI_HD __host__ __device__
#else
#define AV1MI_HD
#endif
#endif

#ifndef AV1MI_PI_K
#define AV1MI_PI_K 3              /* the split penalty's shift (DESIGN §3 item 2c has the sweep, made with -DAV1MI_PI_K=k builds) */
#endif
#define AV1MI_PI_INF 0xFFFFFFFFu  /* cost of a node without a valid candidate */
#define AV1MI_PI_NODES 85         /* 1 + 4 + 16 + 64 */

// Nodes of a superblock in heap order: 0 the 64x64 node, 1 .. 4 the 32x32 nodes, 5 .. 20 the 16x16 nodes, 21 .. 84 the 8x8 nodes, each
// level in Z order - node i's children are 4 i + 1 .. 4 i + 4 (Z order: left to right, then down), and for i < 21 the node's mask bit is i.
enum { AV1MI_PI_OUT = 0, AV1MI_PI_LEAF = 1, AV1MI_PI_MUST = 2, AV1MI_PI_SPLIT = 3, AV1MI_PI_KEEP = 4 };

AV1MI_HD inline uint32_t av1mi_pi_add(uint32_t a, uint32_t b) { return a == AV1MI_PI_INF || b == AV1MI_PI_INF ? AV1MI_PI_INF : a + b; }
AV1MI_HD inline uint32_t av1mi_pi_penalty(int n, int ac_q) { return ((uint32_t)(n * n) * (uint32_t)(ac_q >> 4)) >> AV1MI_PI_K; }

// The search's node tables (me_kernel.hip, node mode): per frame the 32-bit node keys (me_rule.h) of the 8x8 nodes [b8_rows][b8_cols],
// then of the 16x16 and of the 32x32 nodes, a grid each that covers the 8x8 one; all-ones where no candidate was valid.
AV1MI_HD inline int av1mi_pi_level_dim(int b8, int bsl) { return (b8 + (1 << (bsl - 3)) - 1) >> (bsl - 3); }
AV1MI_HD inline size_t av1mi_pi_level_off(int b8_rows, int b8_cols, int bsl) {
  size_t off = 0;
  for (int l = 3; l < bsl; l++) off += (size_t)av1mi_pi_level_dim(b8_rows, l) * av1mi_pi_level_dim(b8_cols, l);
  return off;
}
AV1MI_HD inline size_t av1mi_pi_frame_nodes(int b8_rows, int b8_cols) { return av1mi_pi_level_off(b8_rows, b8_cols, 6); }
// ... and the node of size 2^bsl at frame position (x, y), which must lie inside the frame
AV1MI_HD inline size_t av1mi_pi_node_slot(int b8_rows, int b8_cols, int bsl, int x, int y) {
  return av1mi_pi_level_off(b8_rows, b8_cols, bsl) + (size_t)(y >> bsl) * av1mi_pi_level_dim(b8_cols, bsl) + (x >> bsl);
}

// superblock-local origin and log2 size of node i
AV1MI_HD inline void av1mi_pi_node_pos(int i, int *ox, int *oy, int *bsl) {
  const int level = i < 1 ? 0 : (i < 5 ? 1 : (i < 21 ? 2 : 3));
  const int z = i - (level == 0 ? 0 : (level == 1 ? 1 : (level == 2 ? 5 : 21)));
  int x = 0, y = 0;
  for (int d = 0; d < level; d++) {   // base-4 digit d of z, least significant first = the step of size 64 >> (level - d)
    const int q = (z >> (2 * d)) & 3, step = 64 >> (level - d);
    x += (q & 1) * step; y += (q >> 1) * step;
  }
  *ox = x; *oy = y; *bsl = 6 - level;
}

// One node at frame position (x, y): its J and its state from its own cL and its children's J (children outside the frame are skipped;
// childJ is not read for an 8x8 node).
AV1MI_HD inline uint32_t av1mi_pi_node(int width, int height, int min_bs_log2, int max_bs_log2, int ac_q, int x, int y, int bsl,
                                       uint32_t cL, const uint32_t *childJ, int *state) {
  const int n = 1 << bsl, h = n >> 1;
  if (x >= width || y >= height) { *state = AV1MI_PI_OUT; return 0; }
  if (bsl <= 3) { *state = AV1MI_PI_LEAF; return cL; }
  uint32_t sum = 0;
  for (int q = 0; q < 4; q++)
    if (x + (q & 1) * h < width && y + (q >> 1) * h < height) sum = av1mi_pi_add(sum, childJ[q]);
  if (y + h >= height || x + h >= width) { *state = AV1MI_PI_MUST; return sum; }
  if (bsl <= min_bs_log2) { *state = AV1MI_PI_LEAF; return cL; }
  if (bsl > max_bs_log2) { *state = AV1MI_PI_MUST; return sum; }
  const uint32_t S = av1mi_pi_add(sum, av1mi_pi_penalty(n, ac_q));
  if (S < cL) { *state = AV1MI_PI_SPLIT; return S; }
  *state = AV1MI_PI_KEEP; return cL;
}

// Is node i reached - do all its ancestors split?  (state[] of every node, from av1mi_pi_node.)
AV1MI_HD inline int av1mi_pi_reached(const uint8_t *state, int i) {
  if (state[i] == AV1MI_PI_OUT) return 0;
  while (i > 0) {
    i = (i - 1) >> 2;
    if (state[i] != AV1MI_PI_MUST && state[i] != AV1MI_PI_SPLIT) return 0;
  }
  return 1;
}

// The whole superblock at (sb_x, sb_y): the canonical mask; leaf[i] = 1 where node i is a leaf of the decided tree.
AV1MI_HD inline uint32_t av1mi_pi_decide_sb(int width, int height, int min_bs_log2, int max_bs_log2, int ac_q, int sb_x, int sb_y,
                                            const uint32_t *cL /* [85] */, uint8_t *leaf /* [85] */) {
  uint32_t J[AV1MI_PI_NODES];
  uint8_t state[AV1MI_PI_NODES];
  for (int i = AV1MI_PI_NODES - 1; i >= 0; i--) {
    int ox, oy, bsl, st;
    av1mi_pi_node_pos(i, &ox, &oy, &bsl);
    J[i] = av1mi_pi_node(width, height, min_bs_log2, max_bs_log2, ac_q, sb_x + ox, sb_y + oy, bsl, cL[i], i < 21 ? &J[4 * i + 1] : nullptr, &st);
    state[i] = (uint8_t)st;
  }
  uint32_t mask = 0;
  for (int i = 0; i < AV1MI_PI_NODES; i++) {
    const int r = av1mi_pi_reached(state, i);
    leaf[i] = (uint8_t)(r && (state[i] == AV1MI_PI_LEAF || state[i] == AV1MI_PI_KEEP));
    if (r && state[i] == AV1MI_PI_SPLIT) mask |= 1u << i;
  }
  return mask;
}
#endif
