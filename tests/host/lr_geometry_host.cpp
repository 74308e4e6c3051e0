// The restoration units' geometry header (av1-base_amd/csrc/lr_geometry.h) compiled for the host: tests/test_lr_unit_host.py checks the
// counts, the bounds, the cell -> unit map and the coding superblock against the Python restatement (tests/lr_ref.py, tests/lr_unit_ref.py)
// through the functions below, and runs the stand-alone program (-DLR_GEOMETRY_MAIN) plain and under the sanitizers: for every even size
// 8 .. 1200 and every shift it proves, from the header alone, what the kernels rely on.
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

static long g_checks = 0, g_fail = 0;
static void check(bool ok, const char *what, int size, int shift, int a, int b) {
  g_checks++;
  if (!ok && g_fail++ < 20) printf("FAIL %s: size %d shift %d (%d, %d)\n", what, size, shift, a, b);
}

int main() {
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
