// Host-side check of the symbolize launcher's geometry (av1mi_dev.h: av1mi_tile_is_regular, av1mi_edge_tile), built as plain C++ by
// tests/test_chunk_path_host.py: without a partition map every tile of the full variant is one of the frame's edge tiles, the edge
// tiles are distinct tiles of the grid, and a named geometry has (or has not) a full-variant tile at all.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../av1-base_amd/csrc/av1mi_dev.h"

static Av1miDevParams params_of(int w, int h, int leaf_log2, int tsb, int static_cdfs) {
  Av1miDevParams P;
  memset(&P, 0, sizeof(P));
  P.width = w; P.height = h; P.sb_cols = (w + 63) / 64; P.sb_rows = (h + 63) / 64; P.tile_sb = tsb;
  P.tile_cols = (P.sb_cols + tsb - 1) / tsb; P.tile_rows = (P.sb_rows + tsb - 1) / tsb;
  P.max_bs_log2 = P.min_bs_log2 = leaf_log2; P.disable_cdf_update = static_cdfs;
  return P;
}

// number of full-variant tiles of a frame, or -1 if one of them is not an edge tile / the edge tiles are not distinct tiles
static int full_tiles(const Av1miDevParams &P) {
  const int nt = P.tile_rows * P.tile_cols;
  std::set<int> edge;
  for (int e = 0; e < av1mi_edge_tiles(P); e++) {
    const int t = av1mi_edge_tile(P, e);
    if (t < 0 || t >= nt || !edge.insert(t).second) return -1;
  }
  int n = 0;
  for (int t = 0; t < nt; t++)
    if (!av1mi_tile_is_regular(P, 0, t / P.tile_cols, t % P.tile_cols, P.tile_sb)) {
      if (!edge.count(t)) return -1;
      n++;
    }
  return n;
}

int main(int argc, char **argv) {
  if (argc == 6) {   // width height leaf_log2 tile_sb static_cdfs -> the count
    printf("%d\n", full_tiles(params_of(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]))));
    return 0;
  }
  long checked = 0;
  for (int tsb = 1; tsb <= 2; tsb++)
    for (int L = 3; L <= 6; L++)
      for (int w = 8; w <= 400; w += 8)
        for (int h = 8; h <= 400; h += 8) {
          if (full_tiles(params_of(w, h, L, tsb, 0)) < 0) { printf("%dx%d leaf %d tile_sb %d: a full-variant tile outside the edge tiles\n", w, h, L, tsb); return 1; }
          checked++;
        }
  printf("ok %ld\n", checked);
  return 0;
}
