// lr_geometry.h - the grid of loop restoration units at a unit size (av1mi_params.enable_lr bits 12-13, lr_unit_shift; DESIGN.md §3 item
// 9f), for host and device: the restoration kernels, symbolize's read_lr and the host code take their counts, bounds and maps from here,
// tests/host/lr_geometry_host.cpp compiles it for the CPU against tests/lr_ref.py.  Normative: §5.9.20 (unit sizes), §5.11.57 (which
// superblock reads which unit), §7.17 (count_units_in_frame, the units' bounds, the row offset of 8 luma rows).
//
//   unit size    U = 64 << shift luma samples, shift 0 .. 2; lr_uv_shift = 1, so a chroma unit is U / 2 chroma samples - the picture area
//                of a luma unit.  The signalled size is even: the three planes share one grid, counted on the luma size
//   count        max((size + U / 2) / U, 1) per direction
//   rows         unit row R covers plane rows R U - 8 .. (R + 1) U - 9 (chroma: halved), row 0 from 0, the last row to the plane's end
//   columns      C U .. (C + 1) U - 1 (chroma: halved), the last column to the plane's end
//   cells        the units of shift 0.  They are the kernels' work items at every shift: cell (r, c) lies wholly inside unit
//                (min(r >> shift, rows - 1), min(c >> shift, cols - 1)), and cell (R << shift, C << shift) is the unit's first
//   coding       unit (R, C) of every restored plane is read with superblock (R << shift, C << shift)
#ifndef AV1MI_LR_GEOMETRY_H
#define AV1MI_LR_GEOMETRY_H
#ifdef __HIPCC__
#define AV1MI_GEO_HD __host__ __device__
#else
#define AV1MI_GEO_HD
#endif

#define AV1MI_LR_MAX_UNIT_SHIFT 2

// count_units_in_frame (§7.17) of `size` luma samples
AV1MI_GEO_HD inline int av1mi_lr_count(int size, int shift) {
  const int U = 64 << shift, n = (size + (U >> 1)) / U;
  return n > 0 ? n : 1;
}
// first and one-past-last row of unit row `r` of `n` in a plane of `h` rows (sub = 1: chroma), and the same for columns
AV1MI_GEO_HD inline int av1mi_lr_row0(int r, int shift, int sub) { return r ? (r * (64 << shift) - 8) >> sub : 0; }
AV1MI_GEO_HD inline int av1mi_lr_row1(int r, int n, int shift, int sub, int h) { return r == n - 1 ? h : ((r + 1) * (64 << shift) - 8) >> sub; }
AV1MI_GEO_HD inline int av1mi_lr_col0(int c, int shift, int sub) { return (c * (64 << shift)) >> sub; }
AV1MI_GEO_HD inline int av1mi_lr_col1(int c, int n, int shift, int sub, int w) { return c == n - 1 ? w : ((c + 1) * (64 << shift)) >> sub; }
// the unit (of `units` in its direction) that cell `cell` belongs to, and the unit's first cell
AV1MI_GEO_HD inline int av1mi_lr_unit_of_cell(int cell, int units, int shift) {
  const int u = cell >> shift;
  return u < units ? u : units - 1;
}
AV1MI_GEO_HD inline int av1mi_lr_first_cell(int unit, int shift) { return unit << shift; }
// the superblock row / column a unit is coded with, and the unit a superblock row / column reads: -1 if none starts there
AV1MI_GEO_HD inline int av1mi_lr_unit_sb(int unit, int shift) { return unit << shift; }
AV1MI_GEO_HD inline int av1mi_lr_sb_unit(int sb, int units, int shift) {
  if (sb & ((1 << shift) - 1)) return -1;
  return (sb >> shift) < units ? sb >> shift : -1;
}

#endif
