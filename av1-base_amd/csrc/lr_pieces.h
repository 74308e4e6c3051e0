// lr_pieces.h - what the loop restoration kernels share (lr_kernel.hip: the fixed candidates; lr_fit_kernel.hip: the self-guided fit):
// the candidate tables, a wave's LDS tiles, the staged source window, the Wiener filter and the wave reductions.  Device code only;
// included inside each translation unit's unnamed namespace, so each has its own LDS and constants.
// LDS per wave: window 3.1 KB + Wiener tile 3.1 KB + self-guided grids 10.7 KB.

__constant__ int8_t c_wiener_cand[3][3] = { { 0, 0, -4 }, { 1, -3, -6 }, { 3, -7, 15 } };
// chroma (enable_lr = 3 / 4): §5.11.58 codes taps 1 and 2 of a chroma filter, tap 0 is 0
__constant__ int8_t c_wiener_cand_uv[3][3] = { { 0, 0, -4 }, { 0, 0, 16 }, { 0, 6, 20 } };  // == av1mi_host.cpp kWienerCandUV

// a wave works on at most 16 rows (LR_SLICES): the source window of those rows (3 more above, 2..3 below, 3 columns either
// side; get_source_sample's stripe rule applied per row) is staged once and both filters read it from LDS
__shared__ uint16_t g_win[22][72];
__shared__ int16_t g_mid[22][72];   // Wiener: horizontal-pass output [row][lane]

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// horizontal pass of rows [ya - 3, yb + 3) for column xs + lane, from the staged window, into g_mid[row - (ya - 3)][lane]
__device__ __forceinline__ void wiener_h(int bd, int ya, int yb, const int *f, int lane) {
  const int offset = 1 << (bd + 7 - 3 - 1), limit = (1 << (bd + 1 + 7 - 3)) - 1;
  for (int r = 0; r < yb - ya + 6; r++) {
    int s = 0;
#pragma unroll
    for (int t = 0; t < 7; t++) s += f[t] * (int)g_win[r][lane + t];
    g_mid[r][lane] = (int16_t)clampi((s + 4) >> 3, -offset, limit - offset);
  }
}
__device__ __forceinline__ int wiener_v(int row_in_mid, int lane, const int *f, int maxv) {
  int s = 0;
#pragma unroll
  for (int t = 0; t < 7; t++) s += f[t] * (int)g_mid[row_in_mid + t][lane];
  return clampi((s + 1024) >> 11, 0, maxv);
}
__device__ __forceinline__ void taps_of(int k, int *f) {
  const int c0 = c_wiener_cand[k][0], c1 = c_wiener_cand[k][1], c2 = c_wiener_cand[k][2];
  f[0] = f[6] = c0; f[1] = f[5] = c1; f[2] = f[4] = c2; f[3] = 128 - 2 * (c0 + c1 + c2);
}
__device__ __forceinline__ void taps_of_uv(int k, int *f) {
  const int c1 = c_wiener_cand_uv[k][1], c2 = c_wiener_cand_uv[k][2];
  f[0] = f[6] = 0; f[1] = f[5] = c1; f[2] = f[4] = c2; f[3] = 128 - 2 * (c1 + c2);
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// lanes 0-31 get the sum of lanes 0-31, lanes 32-63 that of lanes 32-63 (two chroma units side by side)
__device__ __forceinline__ unsigned long long half_sum64(unsigned long long v) {
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- self-guided restoration (enable_lr = 2; §7.17.3 self guided filter process / box filter process) ---------------
// Candidates (oracle/av1o_lr.c av1o_sgr_candidates): parameter set 9 (pass 0: r = 2, eps 68; pass 1: r = 1, eps 15) with the
// weights (xqd0, xqd1) = (31, 31), (0, 31), (31, 95): both box-filter passes are computed once per sample, the candidates
// differ only in the final blend.
__constant__ int8_t c_sgr_cand[3][3] = { { 9, 31, 31 }, { 9, 0, 31 }, { 9, 31, 95 } };
// A (<= 256) and B of the box filter at the positions a slice of SGR_ROWS rows of a unit section needs: rows ya - 1 .. yb
// (<= SGR_ROWS + 2), columns xs - 1 .. xs + 64.  Slices keep the LDS footprint small (whole 64-row sections
// needed 62 KB: 2 waves per CU, half the SIMDs idle, 3x slower).
#define SGR_ROWS 16   /* == the rows of a wave's slice */
// Pass 0 (r = 2) is only evaluated at odd rows: its grids hold every second row (row index >> 1; a slice starts at an even row, so
// the odd rows ya - 1, ya + 1 .. have even indices).  That is 3.5 KB less: 17 KB per wave, 9 waves per CU instead of 7, and the
// 2040 working waves of a 1080p frame are resident at once (the same step the inter pass took).
__shared__ uint16_t g_sgrA0[(SGR_ROWS + 2) / 2][66], g_sgrA1[SGR_ROWS + 2][66];
__shared__ int32_t g_sgrB0[(SGR_ROWS + 2) / 2][66], g_sgrB1[SGR_ROWS + 2][66];

// get_source_sample (§7.17.6): the row of a plane of H rows that supplies restoration input row y of the stripe [s0, s1]
template <typename PIX>
__device__ __forceinline__ const PIX *lr_row(const PIX *cdef, const PIX *pre, int y, int s0, int s1, int H, int stride) {
  int yy = clampi(y, 0, H - 1);
  const PIX *fr = cdef;
  if (yy < s0) { yy = yy > s0 - 2 ? yy : s0 - 2; fr = pre; }
  else if (yy > s1) { yy = yy < s1 + 2 ? yy : s1 + 2; fr = pre; }
  return fr + (size_t)yy * stride;
}

// Source window of a unit section for the box sums: restoration input rows ya - 3 .. yb + 2 (get_source_sample's stripe rule
// per row), columns xs - 3 .. xs + 66 (clamped to the plane of W x H samples) -> win[row - (ya - 3)][col - (xs - 3)], all loads
// independent.
template <typename PIX>
__device__ __forceinline__ void lr_stage(const PIX *cdef, const PIX *pre, int xs, int ya, int yb, int s0, int s1, int W, int H, int stride,
                                         int lane) {
  uint16_t (*win)[72] = g_win;
  const int rows = yb - ya + 6;
#pragma unroll 8
  for (int p = lane; p < rows * 70; p += 64) {
    const int i = p / 70, j = p - i * 70;
    win[i][j] = (uint16_t)lr_row<PIX>(cdef, pre, ya - 3 + i, s0, s1, H, stride)[clampi(xs - 3 + j, 0, W - 1)];
  }
}

// A cell (a unit of lr_unit_shift 0) is LR_SLICES waves, one per 16 of its rows (the last cell of a column has up to 103); a pair of
// chroma cells LR_SLICES_C (up to 51 rows).  av1mi_dev.h's av1mi_lr_grid sizes the launches with them.
#define LR_SLICES AV1MI_LR_SLICES
#define LR_SLICES_C AV1MI_LR_SLICES_C
