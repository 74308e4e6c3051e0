// The inter frames' partition rule (av1-base_amd/csrc/part_inter_rule.h: what inter_partition_kernel runs) compiled for the host, for
// tests/test_part_inter_host.py: reads superblocks from a text file - one per line: width height min_bs_log2 max_bs_log2 ac_q sb_x sb_y and
// the 85 node costs in heap order (4294967295 = no valid candidate) - and prints per line the mask and the 85 leaf flags.  Decided twice:
// by av1mi_pi_decide_sb and level by level through av1mi_pi_node / av1mi_pi_reached as the kernel's lanes do; the two must agree.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../av1-base_amd/csrc/part_inter_rule.h"

static uint32_t by_levels(int W, int H, int lo, int hi, int acq, int sb_x, int sb_y, const uint32_t *cL, uint8_t *leaf) {
  uint32_t J[AV1MI_PI_NODES];
  uint8_t state[AV1MI_PI_NODES];
  static const int first[4] = {21, 5, 1, 0}, count[4] = {64, 16, 4, 1};
  for (int level = 0; level < 4; level++)
    for (int i = first[level]; i < first[level] + count[level]; i++) {
      int ox, oy, bsl, st;
      av1mi_pi_node_pos(i, &ox, &oy, &bsl);
      if (bsl != 3 + level) return 0xFFFFFFFFu;
      J[i] = av1mi_pi_node(W, H, lo, hi, acq, sb_x + ox, sb_y + oy, bsl, cL[i], i < 21 ? &J[4 * i + 1] : nullptr, &st);
      state[i] = (uint8_t)st;
    }
  uint32_t mask = 0;
  for (int i = 0; i < AV1MI_PI_NODES; i++) {
    const int r = av1mi_pi_reached(state, i);
    leaf[i] = (uint8_t)(r && (state[i] == AV1MI_PI_LEAF || state[i] == AV1MI_PI_KEEP));
    if (i < 21 && r && state[i] == AV1MI_PI_SPLIT) mask |= 1u << i;
  }
  return mask;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int W, H, lo, hi, acq, sb_x, sb_y;
  long n = 0, disagree = 0;
  while (fscanf(f, "%d %d %d %d %d %d %d", &W, &H, &lo, &hi, &acq, &sb_x, &sb_y) == 7) {
    uint32_t cL[AV1MI_PI_NODES];
    for (int i = 0; i < AV1MI_PI_NODES; i++) {
      unsigned long v;
      if (fscanf(f, "%lu", &v) != 1) { fprintf(stderr, "short line %ld\n", n); fclose(f); return 2; }
      cL[i] = (uint32_t)v;
    }
    uint8_t leaf[AV1MI_PI_NODES], leaf2[AV1MI_PI_NODES];
    const uint32_t mask = av1mi_pi_decide_sb(W, H, lo, hi, acq, sb_x, sb_y, cL, leaf);
    const uint32_t mask2 = by_levels(W, H, lo, hi, acq, sb_x, sb_y, cL, leaf2);
    if (mask != mask2 || memcmp(leaf, leaf2, sizeof(leaf))) disagree++;
    printf("%u ", mask);
    for (int i = 0; i < AV1MI_PI_NODES; i++) putchar('0' + leaf[i]);
    putchar('\n');
    n++;
  }
  fclose(f);
  fprintf(stderr, "%ld superblocks, %ld disagreements\n", n, disagree);
  return disagree ? 1 : 0;
}
