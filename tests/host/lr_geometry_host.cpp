// The restoration units' geometry header (av1-base_amd/csrc/lr_geometry.h) compiled for the host: tests/test_lr_unit_host.py checks the
// counts, the bounds, the cell -> unit map and the coding superblock against the Python restatement (tests/lr_ref.py, tests/lr_unit_ref.py)
// through the functions below, and runs the stand-alone program (-DLR_GEOMETRY_MAIN) plain and under the sanitizers: for every even size
// 8 .. 1200 and every shift it proves, from the header alone, what the kernels rely on - and, for the two fits' blocks of per-unit tables
// (av1mi_dev.h: av1mi_lr_fit_split, av1mi_lr_wfit_split), that the parts fill a block of av1mi_lr_*fit_bytes without touching each other.
#include "../../av1-base_amd/csrc/lr_geometry.h"

extern "C" int geo_count(int size, int shift) { return av1mi_lr_count(size, shift); }
// out[2 n]: first and one-past-last row of every unit row of a plane of `h` rows (h = the luma size >> sub), then the same call with
// cols = 1 gives the columns
extern "C" void geo_bounds(int luma_size, int shift, int sub, int cols, int *out) {
  const int n = av1mi_lr_count(luma_size, shift), size = (luma_size + sub) >> sub;
  for (int u = 0; u < n; u++) {
    out[2 * u] = cols ? av1mi_lr_col0(u, shift, sub) : av1mi_lr_row0(u, shift, sub);
    out[2 * u + 1] = cols ? av1mi_lr_col1(u, n, shift, sub, size) : av1mi_lr_row1(u, n, shift, sub, size);
  }
}
extern "C" int geo_unit_of_cell(int cell, int units, int shift) { return av1mi_lr_unit_of_cell(cell, units, shift); }
extern "C" int geo_first_cell(int unit, int shift) { return av1mi_lr_first_cell(unit, shift); }
extern "C" int geo_unit_sb(int unit, int shift) { return av1mi_lr_unit_sb(unit, shift); }
extern "C" int geo_sb_unit(int sb, int units, int shift) { return av1mi_lr_sb_unit(sb, units, shift); }

#ifdef LR_GEOMETRY_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../av1-base_amd/csrc/av1mi_dev.h"

static long g_checks = 0, g_fail = 0;
static void check(bool ok, const char *what, int size, int shift, int a, int b) {
  g_checks++;
  if (!ok && g_fail++ < 20) printf("FAIL %s: size %d shift %d (%d, %d)\n", what, size, shift, a, b);
}

// a block of exactly the stated size, every part written over its whole extent (the sanitizers see a write past the block), then read
// back: the parts are disjoint, the 64-bit ones aligned, errors and records are the head the host fetches, at_frame strides every part
static bool filled(const void *p, int v, size_t bytes) {
  for (size_t i = 0; i < bytes; i++) if (((const unsigned char *)p)[i] != v) return false;
  return true;
}
static void check_fit_blocks() {
  for (size_t n = 1; n <= 2000; n += n < 24 ? 1 : 97) {
    unsigned char *blk = (unsigned char *)malloc(av1mi_lr_fit_bytes(n));
    const Av1miLrFit F = av1mi_lr_fit_split(blk, n, 0xFFFFu);
    const size_t be = n * AV1MI_LR_FIT_CANDS * 8, br = n * 4, bs = n * AV1MI_LR_FIT_SETS * 5 * 8, bc = n * 2 * 4;
    memset(F.err, 1, be); memset(F.rec, 2, br); memset(F.sums, 3, bs); memset(F.code, 4, bc);
    check(filled(F.err, 1, be) && filled(F.rec, 2, br) && filled(F.sums, 3, bs) && filled(F.code, 4, bc), "self-guided fit: parts disjoint", (int)n, 0, 0, 0);
    check((unsigned char *)F.err == blk && (unsigned char *)F.rec == blk + be && (unsigned char *)F.rec + br == blk + av1mi_lr_fit_result_bytes(n),
          "self-guided fit: the fetched head", (int)n, 0, 0, 0);
    check(((size_t)((unsigned char *)F.sums - blk) & 7) == 0 && (unsigned char *)F.code + bc <= blk + av1mi_lr_fit_bytes(n) && F.mask == 0xFFFFu,
          "self-guided fit: alignment and end", (int)n, 0, 0, 0);
    const Av1miLrFit G = F.at_frame(0, n).at_frame(1, n / 2);
    check(G.err == F.err + n / 2 * AV1MI_LR_FIT_CANDS && G.rec == F.rec + n / 2 * 4 && G.sums == F.sums + n / 2 * AV1MI_LR_FIT_SETS * 5 &&
          G.code == F.code + n / 2 * 2 && G.mask == F.mask, "self-guided fit: at_frame", (int)n, 0, 0, 0);
    free(blk);
    blk = (unsigned char *)malloc(av1mi_lr_wfit_bytes(n));
    const Av1miLrWfit W = av1mi_lr_wfit_split(blk, n);
    const size_t we = n * 8, wr = n * 8, ws = n * AV1MI_LR_WFIT_SUMS * 8, wc = n * 3 * 4;
    memset(W.err, 1, we); memset(W.rec, 2, wr); memset(W.sums, 3, ws); memset(W.code, 4, wc);
    check(filled(W.err, 1, we) && filled(W.rec, 2, wr) && filled(W.sums, 3, ws) && filled(W.code, 4, wc), "Wiener fit: parts disjoint", (int)n, 0, 0, 0);
    check((unsigned char *)W.err == blk && (unsigned char *)W.rec + wr == blk + av1mi_lr_wfit_result_bytes(n) &&
          (unsigned char *)W.code + wc == blk + av1mi_lr_wfit_bytes(n), "Wiener fit: head and end", (int)n, 0, 0, 0);
    const Av1miLrWfit V = W.at_frame(1, n / 2);
    check(V.err == W.err + n / 2 && V.rec == W.rec + n / 2 * 8 && V.sums == W.sums + n / 2 * AV1MI_LR_WFIT_SUMS && V.code == W.code + n / 2 * 3,
          "Wiener fit: at_frame", (int)n, 0, 0, 0);
    free(blk);
  }
}

int main() {
  check_fit_blocks();
  for (int size = 8; size <= 1200; size += 2)
    for (int shift = 0; shift <= AV1MI_LR_MAX_UNIT_SHIFT; shift++) {
      const int U = 64 << shift, units = av1mi_lr_count(size, shift), cells = av1mi_lr_count(size, 0);
      const int sbs = (((size + 7) & ~7) + 63) / 64;   // superblocks of the coded size
      if (shift == 0) check(units == ((size + 32) / 64 > 0 ? (size + 32) / 64 : 1), "the grid of 64x64 units", size, shift, units, 0);
      check(units >= 1 && units <= cells, "count", size, shift, units, cells);
      for (int sub = 0; sub < 2; sub++) {
        const int plane = (size + sub) >> sub;
        // the units tile the plane, rows and columns; the last is at most 1.5 U - 1 wide and 1.5 U + 7 tall
        int at_r = 0, at_c = 0;
        for (int u = 0; u < units; u++) {
          const int r0 = av1mi_lr_row0(u, shift, sub), r1 = av1mi_lr_row1(u, units, shift, sub, plane);
          const int c0 = av1mi_lr_col0(u, shift, sub), c1 = av1mi_lr_col1(u, units, shift, sub, plane);
          check(r0 == at_r && r1 > r0, "rows tile", size, shift, u, r0);
          check(c0 == at_c && c1 > c0, "columns tile", size, shift, u, c0);
          check(r0 == (u ? (u * U - 8) >> sub : 0) && (u == units - 1 || r1 == ((u + 1) * U - 8) >> sub), "row bounds", size, shift, u, r1);
          check(c0 == (u * U) >> sub && (u == units - 1 || c1 == ((u + 1) * U) >> sub), "column bounds", size, shift, u, c1);
          check(c1 - c0 <= ((3 * U / 2 - 1) >> sub) + sub && r1 - r0 <= ((3 * U / 2 + 7) >> sub) + sub, "extent", size, shift, c1 - c0, r1 - r0);
          at_r = r1; at_c = c1;
        }
        check(at_r == plane && at_c == plane, "the units end with the plane", size, shift, at_r, at_c);
        // every cell lies wholly inside exactly one unit - the one the map names - and every unit's first cell is its first
        for (int c = 0; c < cells; c++) {
          const int cr0 = av1mi_lr_row0(c, 0, sub), cr1 = av1mi_lr_row1(c, cells, 0, sub, plane);
          const int cc0 = av1mi_lr_col0(c, 0, sub), cc1 = av1mi_lr_col1(c, cells, 0, sub, plane);
          const int u = av1mi_lr_unit_of_cell(c, units, shift);
          int in_rows = 0, in_cols = 0;
          for (int v = 0; v < units; v++) {
            in_rows += cr0 >= av1mi_lr_row0(v, shift, sub) && cr1 <= av1mi_lr_row1(v, units, shift, sub, plane);
            in_cols += cc0 >= av1mi_lr_col0(v, shift, sub) && cc1 <= av1mi_lr_col1(v, units, shift, sub, plane);
          }
          check(in_rows == 1 && in_cols == 1, "a cell in exactly one unit", size, shift, c, in_rows * 10 + in_cols);
          check(u >= 0 && u < units && cr0 >= av1mi_lr_row0(u, shift, sub) && cr1 <= av1mi_lr_row1(u, units, shift, sub, plane) &&
                cc0 >= av1mi_lr_col0(u, shift, sub) && cc1 <= av1mi_lr_col1(u, units, shift, sub, plane), "the map's unit holds the cell", size, shift, c, u);
        }
        for (int u = 0; u < units; u++) {
          const int c = av1mi_lr_first_cell(u, shift);
          check(c < cells && av1mi_lr_unit_of_cell(c, units, shift) == u && (c == 0 || av1mi_lr_unit_of_cell(c - 1, units, shift) == u - 1) &&
                av1mi_lr_row0(c, 0, sub) == av1mi_lr_row0(u, shift, sub) && av1mi_lr_col0(c, 0, sub) == av1mi_lr_col0(u, shift, sub),
                "a unit's first cell", size, shift, u, c);
        }
      }
      // the coding superblock of every unit exists and is distinct; the superblocks' map is its inverse and names no other unit
      int read = 0;
      for (int u = 0; u < units; u++) {
        const int sb = av1mi_lr_unit_sb(u, shift);
        check(sb < sbs && (u == 0 || sb > av1mi_lr_unit_sb(u - 1, shift)) && av1mi_lr_sb_unit(sb, units, shift) == u, "coding superblock", size, shift, u, sb);
        // §5.11.57: the superblock whose rows 64 sb .. 64 sb + 63 hold the unit's nominal origin u U
        check(sb * 64 <= u * U && u * U < sb * 64 + 64, "the unit starts in its superblock", size, shift, u, sb);
      }
      for (int sb = 0; sb < sbs; sb++) {
        const int u = av1mi_lr_sb_unit(sb, units, shift);
        // §5.11.57's own range: unitRowStart = ceil(64 sb / U), unitRowEnd = min(ceil(64 (sb + 1) / U), units)
        const int lo = (sb * 64 + U - 1) / U, hi0 = ((sb + 1) * 64 + U - 1) / U, hi = hi0 < units ? hi0 : units;
        check(hi - lo <= 1 && (hi > lo ? u == lo : u == -1), "read_lr's range", size, shift, sb, u);
        read += u >= 0;
      }
      check(read == units, "every unit is read once", size, shift, read, units);
    }
  printf("%ld checks, %ld failures\n", g_checks, g_fail);
  return g_fail != 0;
}
#endif
