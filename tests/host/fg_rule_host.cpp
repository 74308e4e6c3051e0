// The film-grain estimate's rule (av1-base_amd/csrc/fg_rule.h) compiled for the host, as a stand-alone program: tests/test_fg_host.py
// writes the cases, runs it - plain and under the sanitizers - and checks the lines against the numpy restatement (tests/fg_ref.py).
// Linked with av1-base_amd/csrc/av1mi_syntax.cpp for the frame headers of both kinds.
//   B bd n x[n * n]          a block of n x n samples (n = 16 luma, 8 chroma)   ->  Nsum value bin (bin -1 for chroma)
//   Q n v[n]                 n block values                                     ->  their lower quartile
//   T ceil_y ceil_c n r[n]   n block records bin | v_y << 8 | v_u << 16 | v_v << 24  ->  the 24 table values, then the 24 counts
//   W nbx nby frames grid    the block walk of a chunk by a grid of workgroups  ->  the steps; the luma [block][row] and the chroma
//                            [plane][pair][row] slots visited exactly once, and all visits of either; the chroma visits whose pair has
//                            its right block; what is wrong (a lane's place, a block outside the picture, a `both` that is not
//                            bx + 1 < nbx); lanes whose step count differs from their workgroup's; sum (g + 1) steps of workgroup g;
//                            sum (step * 8 + slot + 1) (block + 1) over the luma visits, modulo 2^64
//   H p[36] frame inter      av1mi_params as 36 words, a frame number, the kind ->  rc, the header's bits, fg_bit, the header in hex
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../av1-base_amd/csrc/av1mi_syntax.h"
#include "../../av1-base_amd/csrc/fg_rule.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'B') {
      int bd, n;
      if (fscanf(f, "%d %d", &bd, &n) != 2 || (n != 8 && n != 16)) return 3;
      std::vector<uint16_t> x((size_t)n * n);
      uint32_t S = 0;
      for (auto &v : x) { unsigned u; if (fscanf(f, "%u", &u) != 1) return 3; v = (uint16_t)u; S += u; }
      const uint32_t nsum = av1mi_fg_nsum(x.data(), (size_t)n, n);
      printf("%u %d %d\n", nsum, av1mi_fg_value(nsum, n == 8, bd), n == 16 ? av1mi_fg_bin(S, bd) : -1);
    } else if (kind == 'Q') {
      unsigned n;
      if (fscanf(f, "%u", &n) != 1 || n == 0) return 3;
      std::vector<uint32_t> hist(256, 0);
      for (unsigned i = 0; i < n; i++) { unsigned u; if (fscanf(f, "%u", &u) != 1 || u > 255) return 3; hist[u]++; }
      printf("%d\n", av1mi_fg_quartile(hist.data(), n));
    } else if (kind == 'T') {
      int ceil_y, ceil_c;
      unsigned n;
      if (fscanf(f, "%d %d %u", &ceil_y, &ceil_c, &n) != 3) return 3;
      std::vector<uint32_t> hist((size_t)AV1MI_FG_TABLE * 256, 0);
      uint32_t count[AV1MI_FG_TABLE] = {};
      int value[AV1MI_FG_TABLE] = {};
      for (unsigned i = 0; i < n; i++) {
        unsigned r;
        if (fscanf(f, "%x", &r) != 1 || (r & 0xFF) >= AV1MI_FG_BINS) return 3;
        for (int pl = 0; pl < 3; pl++) { hist[((size_t)pl * AV1MI_FG_BINS + (r & 0xFF)) * 256 + ((r >> (8 + 8 * pl)) & 0xFF)]++; count[pl * AV1MI_FG_BINS + (r & 0xFF)]++; }
      }
      for (int t = 0; t < AV1MI_FG_TABLE; t++) value[t] = count[t] ? av1mi_fg_quartile(hist.data() + (size_t)t * 256, count[t]) : 0;
      for (int t = 0; t < AV1MI_FG_TABLE; t++) {
        const int pl = t / AV1MI_FG_BINS;
        printf("%d ", av1mi_fg_fill(count + pl * AV1MI_FG_BINS, value + pl * AV1MI_FG_BINS, t % AV1MI_FG_BINS, pl ? ceil_c : ceil_y));
      }
      for (int t = 0; t < AV1MI_FG_TABLE; t++) printf("%u%c", count[t], t + 1 < AV1MI_FG_TABLE ? ' ' : '\n');
    } else if (kind == 'W') {
      int nbx, nby, nf, grid;
      if (fscanf(f, "%d %d %d %d", &nbx, &nby, &nf, &grid) != 4 || nbx < 0 || nby < 0 || nf < 1 || grid < 1) return 3;
      const int npx = (nbx + 1) / 2;
      const long steps = av1mi_fg_walk_steps(nf, nbx, nby);
      std::vector<uint16_t> luma((size_t)nf * nby * nbx * 16, 0), chroma((size_t)2 * nf * nby * npx * 8, 0);   // visits per [block][row], [plane][pair][row]
      unsigned long long order = 0, wg_sum = 0;
      long both = 0, bad = 0, uneven = 0;
      for (int g = 0; g < grid; g++) {   // every workgroup of the grid over its steps, every lane of it
        long taken[AV1MI_FG_WALK_THREADS] = {};
        for (long step = g; step < steps; step += grid)
          for (int t = 0; t < AV1MI_FG_WALK_THREADS; t++) {
            const Av1miFgLane L = av1mi_fg_walk_lane(t);
            const Av1miFgSpot b = av1mi_fg_walk_spot(step, L.slot, nf, nbx, nby);
            taken[t]++;
            if (L.luma != (t < 128) || L.slot < 0 || L.slot >= AV1MI_FG_WALK_SLOTS || L.row < 0 || L.row >= (L.luma ? 16 : 8) ||
                (L.luma ? L.plane != 0 : (L.plane != 1 && L.plane != 2) || (L.slot & 1))) { bad++; continue; }
            if (!b.here) { bad += b.both; continue; }
            if (b.f < 0 || b.f >= nf || b.by < 0 || b.by >= nby || b.bx < 0 || b.bx >= nbx) { bad++; continue; }   // outside the picture
            bad += b.both != (b.bx + 1 < nbx);
            const size_t blk = ((size_t)b.f * nby + b.by) * nbx + b.bx;
            if (L.luma) {
              luma[blk * 16 + L.row]++;
              order += (unsigned long long)(step * 8 + L.slot + 1) * (blk + 1);
            } else {
              chroma[((((size_t)(L.plane - 1) * nf + b.f) * nby + b.by) * npx + b.bx / 2) * 8 + L.row]++;
              both += b.both;
            }
          }
        for (int t = 1; t < AV1MI_FG_WALK_THREADS; t++) uneven += taken[t] != taken[0];
        wg_sum += (unsigned long long)(g + 1) * taken[0];
      }
      size_t luma_once = 0, luma_all = 0, chroma_once = 0, chroma_all = 0;
      for (uint16_t v : luma) { luma_once += v == 1; luma_all += v; }
      for (uint16_t v : chroma) { chroma_once += v == 1; chroma_all += v; }
      printf("%ld %zu %zu %zu %zu %ld %ld %ld %llu %llu\n", steps, luma_once, luma_all, chroma_once, chroma_all, both, bad, uneven, wg_sum, order);
    } else if (kind == 'H') {
      uint32_t w[36];
      unsigned frame, inter;
      for (auto &v : w) if (fscanf(f, "%u", &v) != 1) return 3;
      if (fscanf(f, "%u %u", &frame, &inter) != 2) return 3;
      av1mi_params p;
      static_assert(sizeof(p) == sizeof(w), "av1mi_params is 36 words");
      memcpy(&p, w, sizeof(p));
      av1mi::Resolved r;
      memset(&r, 0, sizeof(r));
      const int rc = av1mi::resolve(&p, &r);
      if (rc) { printf("%d\n", rc); continue; }
      size_t bits = 0, fg_bit = 0;
      const std::vector<uint8_t> h = av1mi::make_frame_header(r, &bits, frame, inter != 0, nullptr, nullptr, &fg_bit);
      printf("0 %zu %zu ", bits, fg_bit);
      for (uint8_t b : h) printf("%02x", b);
      printf("\n");
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
