// lr_pieces.h - what the three loop restoration files share (lr_kernel.hip: the fixed candidates; lr_fit_kernel.hip: the self-guided
// fit; lr_wfit_kernel.hip: the Wiener fit): the candidate tables, a wave's LDS tiles, the staged source window, the Wiener filter, the
// box filter with the strength as an argument, the decision over the fixed candidates, the tail of the applying phase, the reductions
// and the launchers' head; for the two fit files also the stripes, the wave and its sections, and the code kernels' walk (lr_unit_kernel
// and lr_chroma keep their own index arithmetic and stripe loops).  Included inside each translation unit's
// unnamed namespace (after av1mi_dev.h, av1mi_launch.h and lr_rate_rule.h, whose rate term the decision weighs), so each has its own LDS
// and constants.
// LDS per wave: window 3.1 KB + Wiener tile 3.1 KB + self-guided grids 10.7 KB.

// the fixed candidates (lr_fit_rule.h)
__constant__ int8_t c_wiener_cand[3][3] = AV1MI_WIENER_CAND;
__constant__ int8_t c_wiener_cand_uv[3][3] = AV1MI_WIENER_CAND_UV;

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
// the seven taps of a pass from its three coded ones
__device__ __forceinline__ void taps7(int c0, int c1, int c2, int *f) {
  f[0] = f[6] = c0; f[1] = f[5] = c1; f[2] = f[4] = c2; f[3] = 128 - 2 * (c0 + c1 + c2);
}
__device__ __forceinline__ void taps_of(int k, int *f) { taps7(c_wiener_cand[k][0], c_wiener_cand[k][1], c_wiener_cand[k][2], f); }
__device__ __forceinline__ void taps_of_uv(int k, int *f) { taps7(0, c_wiener_cand_uv[k][1], c_wiener_cand_uv[k][2], f); }   // tap 0 is 0
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// lanes 0-31 get the sum of lanes 0-31, lanes 32-63 that of lanes 32-63 (two chroma units side by side)
__device__ __forceinline__ unsigned long long half_sum64(unsigned long long v) {
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the rate terms of a plane's fixed candidates (lr_rate_rule.h): B16 of off, Wiener 1..3 and self-guided 1..3 - the type symbol under the
// frames' restoration type plus the length of the host's bit string against the tile-start reference - and of the two fitted kinds the
// type symbol alone; lambda = 0: the decisions go by the error alone
struct LrRate {
  unsigned long long lambda;
  int b16[7], t16_wiener, t16_sgr;
};
__device__ __forceinline__ LrRate lr_rate(const Av1miDevParams &P, int sub) {
  const int sw = P.enable_lr == 2;
  LrRate R;
  R.lambda = P.lr_lambda;
  R.t16_wiener = av1mi_lr_type_t16(sw, 1); R.t16_sgr = av1mi_lr_type_t16(sw, 2);
  R.b16[0] = av1mi_lr_type_t16(sw, 0);
  for (int k = 0; k < 3; k++) {
    R.b16[1 + k] = av1mi_lr_b16(sub ? P.lr_code_len_uv[0][k] : P.lr_code_len[0][k], R.t16_wiener);
    R.b16[4 + k] = av1mi_lr_b16(P.sgr_code_len[0][k], R.t16_sgr);
  }
  return R;
}

// the decision of a unit over the fixed candidates from its sums: the first minimum of J = 16 D + lambda B16 in the order off, Wiener 1..3
// and (ncand = 6) self-guided 1..3; bj: the minimum, for the self-guided fit to go on from
__device__ __forceinline__ int lr_decide(const unsigned long long *usse, int ncand, const LrRate &R, unsigned long long &bj) {
  int best = 0;
  bj = av1mi_lr_j(usse[0], R.lambda, R.b16[0]);
  for (int k = 0; k < ncand; k++) {
    const unsigned long long j = av1mi_lr_j(usse[k + 1], R.lambda, R.b16[k + 1]);
    if (j < bj) { bj = j; best = k + 1; }
  }
  return best;
}

// ---- self-guided restoration (enable_lr = 2; §7.17.3 self guided filter process / box filter process) ---------------
// Fixed candidates (oracle/av1o_lr.c av1o_sgr_candidates): parameter set 9 (pass 0: r = 2, eps 68; pass 1: r = 1, eps 15) with the
// weights (xqd0, xqd1) = (31, 31), (0, 31), (31, 95): both box-filter passes are computed once per sample, the candidates
// differ only in the final blend.  The self-guided fit runs the same filter with every set's strengths.
__constant__ int8_t c_sgr_cand[3][3] = AV1MI_SGR_CAND;
// A (<= 256) and B of the box filter at the positions a slice of SGR_ROWS rows of a unit section needs: rows ya - 1 .. yb
// (<= SGR_ROWS + 2), columns xs - 1 .. xs + 64.  Slices keep the LDS footprint small (whole 64-row sections
// needed 62 KB: 2 waves per CU, half the SIMDs idle, 3x slower).
#define SGR_ROWS 16   /* == the rows of a wave's slice */
// Pass 0 (r = 2) is only evaluated at odd rows: its grids hold every second row (row index >> 1; a slice starts at an even row, so
// the odd rows ya - 1, ya + 1 .. have even indices).  That is 3.5 KB less: 17 KB per wave, 9 waves per CU instead of 7, and the
// 2040 working waves of a 1080p frame are resident at once (the same step the inter pass took).
__shared__ uint16_t g_sgrA0[(SGR_ROWS + 2) / 2][66], g_sgrA1[SGR_ROWS + 2][66];
__shared__ int32_t g_sgrB0[(SGR_ROWS + 2) / 2][66], g_sgrB1[SGR_ROWS + 2][66];

// A and B from the box sums (sum of samples b, of squares a) of a window of n samples with the strength's scale s = Round(2^20 / (n^2 eps))
__device__ __forceinline__ void box_ab(uint32_t a, uint32_t b, int bd, uint32_t n, uint32_t s, uint32_t one_by_n, uint32_t &A, int32_t &B) {
  const uint32_t a8 = (a + ((1u << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8));
  const uint32_t d = (b + ((1u << (bd - 8)) >> 1)) >> (bd - 8);
  const uint32_t p = a8 * n > d * d ? a8 * n - d * d : 0;
  const uint32_t z = (uint32_t)(((unsigned long long)p * s + (1u << 19)) >> 20);
  const uint32_t a2 = z >= 255 ? 256 : (z == 0 ? 1 : ((z << 8) + z / 2) / (z + 1));
  A = a2;
  B = (int32_t)(((unsigned long long)(256 - a2) * b * one_by_n + (1u << 11)) >> 12);
}

// A/B of pass PASS (radius 2 / 1) with strength eps for the section rows ya - 1 .. yb (<= 18 rows; pass 0 on odd rows only, <= 9) and
// columns xs - 1 .. xs + 64 -> g_sgrA/B[PASS][row - (ya - 1)][col - (xs - 1)], from the staged window (rows ya - 3 .. yb + 2).
// Lane = column xs + lane with a sliding window of row sums; the two edge columns are shared out over the lanes afterwards (direct sums).
template <int PASS>
__device__ __forceinline__ void box_grid(int bd, int ya, int yb, int lane, int eps) {
  constexpr int R = PASS == 0 ? 2 : 1, WN = 2 * R + 1;
  constexpr uint32_t n = WN * WN, one_by_n = ((1u << 12) + n / 2) / n;
  const uint32_t n2e = n * n * (uint32_t)eps, s = ((1u << 20) + n2e / 2) / n2e;
  const uint16_t (*win)[72] = g_win;
  uint32_t h1[WN], h2[WN];   // ring of the last WN row sums
#pragma unroll
  for (int t = 0; t < WN; t++) { h1[t] = 0; h2[t] = 0; }
  for (int yy = ya - 1 - R; yy <= yb + R; yy++) {
    const uint16_t *row = win[yy - (ya - 3)] + lane + 3 - R;
    uint32_t r1 = 0, r2 = 0;
#pragma unroll
    for (int t = 0; t < WN; t++) { const uint32_t c = row[t]; r1 += c; r2 += c * c; }
#pragma unroll
    for (int t = 0; t < WN - 1; t++) { h1[t] = h1[t + 1]; h2[t] = h2[t + 1]; }
    h1[WN - 1] = r1; h2[WN - 1] = r2;
    const int yc = yy - R;   // centre row of the window that just became complete
    if (yc >= ya - 1 && (PASS == 1 || (yc & 1))) {
      uint32_t b = 0, a = 0;
#pragma unroll
      for (int t = 0; t < WN; t++) { b += h1[t]; a += h2[t]; }
      uint32_t A; int32_t B;
      box_ab(a, b, bd, n, s, one_by_n, A, B);
      if (PASS == 0) { g_sgrA0[(yc - (ya - 1)) >> 1][lane + 1] = (uint16_t)A; g_sgrB0[(yc - (ya - 1)) >> 1][lane + 1] = B; }
      else { g_sgrA1[yc - (ya - 1)][lane + 1] = (uint16_t)A; g_sgrB1[yc - (ya - 1)][lane + 1] = B; }
    }
  }
  const int rows = yb - ya + 2;
  for (int task = lane; task < rows * 2; task += 64) {
    const int ri = task >> 1, side = task & 1;
    const int yc = ya - 1 + ri, j = side ? 67 : 2;   // window column of xs + 64 / xs - 1
    if (PASS == 0 && !(yc & 1)) continue;
    uint32_t a = 0, b = 0;
    for (int dy = -R; dy <= R; dy++) {
      const uint16_t *row = win[yc + dy - (ya - 3)] + j - R;
#pragma unroll
      for (int t = 0; t < WN; t++) { const uint32_t c = row[t]; b += c; a += c * c; }
    }
    uint32_t A; int32_t B;
    box_ab(a, b, bd, n, s, one_by_n, A, B);
    if (PASS == 0) { g_sgrA0[ri >> 1][side ? 65 : 0] = (uint16_t)A; g_sgrB0[ri >> 1][side ? 65 : 0] = B; }
    else { g_sgrA1[ri][side ? 65 : 0] = (uint16_t)A; g_sgrB1[ri][side ? 65 : 0] = B; }
  }
}

// box-filter output of the r = 1 pass / the r = 2 pass for sample (xs + lane, y) from the grids; cur = the CDEF sample
__device__ __forceinline__ int box_flt1(int lane, int y, int ya, int cur) {
  const int ri = y - (ya - 1), c = lane + 1;
  int a = 0, b = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int w = (dx == 0 || dy == 0) ? 4 : 3;
      a += w * (int)g_sgrA1[ri + dy][c + dx]; b += w * g_sgrB1[ri + dy][c + dx];
    }
  return (a * cur + b + (1 << 8)) >> 9;
}
__device__ __forceinline__ int box_flt0(int lane, int y, int ya, int cur) {
  const int ri = y - (ya - 1), c = lane + 1;
  int a = 0, b = 0;
  if (y & 1) {  // odd row: the row itself, weights 5 6 5, shift 4
    const int r0 = ri >> 1;
    a = 5 * (int)g_sgrA0[r0][c - 1] + 6 * (int)g_sgrA0[r0][c] + 5 * (int)g_sgrA0[r0][c + 1];
    b = 5 * g_sgrB0[r0][c - 1] + 6 * g_sgrB0[r0][c] + 5 * g_sgrB0[r0][c + 1];
    return (a * cur + b + (1 << 7)) >> 8;
  }
#pragma unroll
  for (int dy = -1; dy <= 1; dy += 2) {  // even row: the rows above and below, shift 5
    const int r0 = (ri + dy) >> 1;
    a += 5 * (int)g_sgrA0[r0][c - 1] + 6 * (int)g_sgrA0[r0][c] + 5 * (int)g_sgrA0[r0][c + 1];
    b += 5 * g_sgrB0[r0][c - 1] + 6 * g_sgrB0[r0][c] + 5 * g_sgrB0[r0][c + 1];
  }
  return (a * cur + b + (1 << 8)) >> 9;
}
// §7.17.3's blend; a pass whose radius is zero contributes u
__device__ __forceinline__ int box_blend(int cur, int r0, int r1, int flt0, int flt1, int w0, int w1, int maxv) {
  const int u = cur << 4, w2 = 128 - w0 - w1;
  const int v = w1 * u + w0 * (r0 ? flt0 : u) + w2 * (r1 ? flt1 : u);
  return clampi((v + (1 << 10)) >> 11, 0, maxv);
}

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

// Stripes (§7.17: StripeStartY = (64 s - 8) >> sub): stripe st of a plane is rows s0 .. s1, 64 >> sub of them - the height of a cell - from
// lr_stripe_row0, offset like the cells by 8 >> sub.  A wave's rows [y0, y1) meet the stripes from lr_first_stripe on while
// lr_stripe_row0 < y1; [ya, yb) is the stripe's section of them (<= 16 rows, ya even).
struct LrStripe { int s0, s1, ya, yb; };
__device__ __forceinline__ int lr_stripe_rows(int sub) { return 64 >> sub; }
__device__ __forceinline__ int lr_stripe_row0(int st, int sub) { return st * lr_stripe_rows(sub) - (8 >> sub); }
__device__ __forceinline__ int lr_first_stripe(int y0, int sub) { return (y0 + (8 >> sub)) / lr_stripe_rows(sub); }
__device__ __forceinline__ LrStripe lr_stripe(int st, int y0, int y1, int sub) {
  const int s0 = lr_stripe_row0(st, sub), s1 = s0 + lr_stripe_rows(sub) - 1;
  return { s0, s1, y0 > s0 ? y0 : s0, y1 < s1 + 1 ? y1 : s1 + 1 };
}

// this lane's CDEF samples (from the staged window) and source samples of a section's rows [ya, yb); rows past yb repeat the last
template <typename PIX>
__device__ __forceinline__ void lr_load_cur_src(const PIX *src, int stride, int x, bool active, int ya, int yb, int lane, int *cur, int *sv) {
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int y = ya + i < yb ? ya + i : yb - 1;
    cur[i] = (int)g_win[y - ya + 3][lane + 3];
    sv[i] = active ? (int)src[(size_t)y * stride + x] : cur[i];
  }
}

// The tail of the phase that writes the reconstruction, for a wave with rows [y0, y1) and columns [x0, x1) of a plane (cdef, out: the
// plane's): the padding between the signalled and the coded size is copied with the last cell of the row / column (its last slice:
// last_row), never filtered, so the whole frame buffer is defined.  copy_chroma (a luma wave of a chunk without chroma restoration;
// cdef, out: the frame's): the co-located chroma, copied as well.
template <typename PIX>
__device__ __forceinline__ void lr_tail(const Av1miDevParams &P, const PIX *cdef, PIX *out, int sub, bool copy_chroma, bool last_row, bool last_col,
                                        int x0, int x1, int y0, int y1, int stride, int lane) {
  const int py1 = last_row ? P.height >> sub : y1, px1 = last_col ? P.width >> sub : x1;
  for (int y = y0; y < py1; y++)
    for (int x = x0 + lane; x < px1; x += 64)
      if (y >= y1 || x >= x1) out[(size_t)y * stride + x] = cdef[(size_t)y * stride + x];
  if (copy_chroma) {
    const int cy0 = y0 >> 1, cy1 = py1 >> 1, cx0 = x0 >> 1, cx1 = px1 >> 1;
    for (int pl = 0; pl < 2; pl++) {
      const size_t po = pl ? P.plane_off_v : P.plane_off_u;
      for (int y = cy0; y < cy1; y++)
        for (int x = cx0 + lane; x < cx1; x += 64) out[po + (size_t)y * P.stride_c + x] = cdef[po + (size_t)y * P.stride_c + x];
    }
  }
}

// A cell (a unit of lr_unit_shift 0) is LR_SLICES waves, one per 16 of its rows (the last cell of a column has up to 103); a pair of
// chroma cells LR_SLICES_C (up to 51 rows).  av1mi_dev.h's av1mi_lr_grid sizes the launches with them.
#define LR_SLICES AV1MI_LR_SLICES
#define LR_SLICES_C AV1MI_LR_SLICES_C

// ---- the fit kernels' wave: block `block` of lr_unit_kernel's grid - luma blocks (cell x LR_SLICES), then with chroma restoration per
// frame and plane cell rows x pairs of cell columns x LR_SLICES_C - as frame f, plane pl (sub: chroma), cell row cr in unit row ur,
// slice, cell column ccl (-1: a chroma pair), columns [x0, x1) (last_col: up to the plane's end), the plane's geometry, rows [y0, y1)
// (last_row: up to the plane's end), and unit (ur, 0) of the plane in the fixed candidates' tables ([frame][restored plane][unit]) and in the
// fits' ([frame][plane 0..2][unit]).  idle: the block has no work.
struct LrWave {
  int f, pl, sub, cr, ur, slice, ccl, x0, x1, last_col, W, H, stride, sh, y0, y1, last_row;
  size_t plane_off, sse_base, fit_base;
  bool idle;
};
__device__ __forceinline__ LrWave lr_wave(const Av1miDevParams &P, unsigned block) {
  const int crows = av1mi_lr_cell_rows(P), ccols = av1mi_lr_cell_cols(P), cells = crows * ccols;
  const int urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int luma_blocks = P.n_frames * cells * LR_SLICES;
  LrWave w;
  if ((int)block < luma_blocks) {
    const int item = block / LR_SLICES, cell = item % cells;
    w.slice = block % LR_SLICES; w.f = item / cells; w.pl = 0; w.cr = cell / ccols; w.ccl = cell % ccols;
    w.x0 = w.ccl * 64; w.last_col = w.ccl == ccols - 1; w.x1 = w.last_col ? P.true_w : w.x0 + 64;
  } else {
    const int item = (int)block - luma_blocks, pairs = (ccols + 1) >> 1, rest = item / LR_SLICES_C;
    const int pc = rest % pairs;
    w.slice = item % LR_SLICES_C; w.cr = rest / pairs % crows; w.pl = 1 + rest / (pairs * crows) % 2; w.f = rest / (pairs * crows * 2); w.ccl = -1;
    w.x0 = pc * 64; w.last_col = pc == pairs - 1; w.x1 = w.last_col ? (P.true_w + 1) >> 1 : w.x0 + 64;
  }
  w.ur = av1mi_lr_unit_of_cell(w.cr, urows, P.lr_unit_shift);
  w.sub = w.pl > 0;
  w.W = w.sub ? (P.true_w + 1) >> 1 : P.true_w; w.H = w.sub ? (P.true_h + 1) >> 1 : P.true_h; w.stride = w.sub ? P.stride_c : P.stride_y;
  w.sh = lr_stripe_rows(w.sub);   // == the cell's size
  w.plane_off = (size_t)w.f * P.frame_samples + (w.pl == 0 ? 0 : (w.pl == 1 ? P.plane_off_u : P.plane_off_v));
  const int uy0 = av1mi_lr_row0(w.cr, 0, w.sub);
  const int uy1 = av1mi_lr_row1(w.cr, crows, 0, w.sub, w.H);   // the cell row's rows
  w.y0 = uy0 + w.slice * 16; w.y1 = w.y0 + 16 < uy1 ? w.y0 + 16 : uy1;
  w.last_row = w.cr == crows - 1 && w.y1 == uy1;
  w.sse_base = ((size_t)w.f * (P.lr_chroma ? 3 : 1) + w.pl) * per + (size_t)w.ur * ucols;
  w.fit_base = ((size_t)w.f * 3 + w.pl) * per + (size_t)w.ur * ucols;
  w.idle = w.y0 >= uy1 || (w.pl && (!P.lr_chroma || w.f >= P.n_frames));
  return w;
}
// the units of the wave's section at column xs: lanes 0-31 are in `lo`, lanes 32-63 in `hi` (one unit: luma, a last chroma cell on its
// own, and two chroma cells of one larger unit); hsel: the lane's half where they differ, unit: the lane's
struct LrSection { int lo, hi, hsel, unit; };
__device__ __forceinline__ LrSection lr_section(const Av1miDevParams &P, const LrWave &w, int xs, int lane) {
  const int ccols = av1mi_lr_cell_cols(P), ucols = av1mi_lr_unit_cols(P);
  LrSection s;
  s.lo = av1mi_lr_unit_of_cell(w.ccl >= 0 ? w.ccl : min(ccols - 1, xs >> 5), ucols, P.lr_unit_shift);
  s.hi = av1mi_lr_unit_of_cell(w.ccl >= 0 ? w.ccl : min(ccols - 1, (xs >> 5) + 1), ucols, P.lr_unit_shift);
  s.hsel = s.lo != s.hi ? lane >> 5 : 0; s.unit = s.hsel ? s.hi : s.lo;
  return s;
}
// is this the lane that writes the section's unit's record: its first column, in the first slice of the unit's first cell
__device__ __forceinline__ bool lr_records(const Av1miDevParams &P, const LrWave &w, int unit, int x, bool active) {
  return w.slice == 0 && w.cr == av1mi_lr_first_cell(w.ur, P.lr_unit_shift) && active && x == av1mi_lr_first_cell(unit, P.lr_unit_shift) * w.sh;
}

// ---- the code kernels' walk: one thread per (frame, restored plane, tile) takes the tile's units in coding order - unit (r, c) of
// every plane is read with superblock (r << lr_unit_shift, c << lr_unit_shift), so a tile may start no unit - and calls
// body(plane, the unit's index in the fits' tables, its index in the fixed candidates'), which carries the plane's references
template <typename BODY>
__device__ __forceinline__ void lr_code_walk(const Av1miDevParams &P, BODY body) {
  const int urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P), per = urows * ucols;
  const int nplanes = P.lr_chroma ? 3 : 1, tiles = P.tile_rows * P.tile_cols;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= P.n_frames * nplanes * tiles) return;
  const int tile = idx % tiles, pl = idx / tiles % nplanes, f = idx / (tiles * nplanes);
  const int tr = tile / P.tile_cols, tc = tile % P.tile_cols, tsb = P.tile_sb;
  for (int si = 0; si < tsb * tsb; si++) {
    const int sbr = tr * tsb + si / tsb, sbc = tc * tsb + si % tsb;
    const int ur = av1mi_lr_sb_unit(sbr, urows, P.lr_unit_shift), uc = av1mi_lr_sb_unit(sbc, ucols, P.lr_unit_shift);
    if (sbr >= P.sb_rows || sbc >= P.sb_cols || ur < 0 || uc < 0) continue;
    body(pl, ((size_t)f * 3 + pl) * per + (size_t)ur * ucols + uc, ((size_t)f * nplanes + pl) * per + (size_t)ur * ucols + uc);
  }
}

// ---- the launchers' head: frames [frame0, frame0 + count) of the chunk - the kernels' parameters, the four frame arrays at frame0,
// the first unit of `choice` and `unit_sse` there, the units of a frame in the fits' tables, the kernels' grid (lr_unit_kernel's for all)
// and the code kernels' threads; lr_launch_typed hands `launch` the frame arrays as the chunk's sample type
struct LrLaunch {
  Av1miDevParams R;
  const void *pre, *cdef, *src;
  void *out;
  size_t upf, unit0, fit_upf;   // units of a frame in choice / unit_sse, the first of frame0 there, units of a frame in the fits' tables
  int grid, code_threads;
};
inline LrLaunch lr_launch_head(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, int frame0, int count) {
  LrLaunch L;
  L.R = av1mi_frame_range(*P, frame0, count);
  L.pre = av1mi_frame_at(L.R, pre, frame0); L.cdef = av1mi_frame_at(L.R, cdef, frame0); L.src = av1mi_frame_at(L.R, src, frame0); L.out = av1mi_frame_at(L.R, out, frame0);
  L.upf = (size_t)av1mi_lr_frame_units(L.R); L.unit0 = frame0 * L.upf;
  L.fit_upf = (size_t)3 * av1mi_lr_unit_rows(L.R) * av1mi_lr_unit_cols(L.R);
  L.grid = av1mi_lr_grid(L.R, count);
  L.code_threads = count * (L.R.lr_chroma ? 3 : 1) * L.R.tile_rows * L.R.tile_cols;
  return L;
}
template <typename LAUNCH>
inline void lr_launch_typed(const LrLaunch &L, LAUNCH launch) {
  if (L.R.bit_depth == 8) launch((const uint8_t *)L.pre, (const uint8_t *)L.cdef, (const uint8_t *)L.src, (uint8_t *)L.out);
  else launch((const uint16_t *)L.pre, (const uint16_t *)L.cdef, (const uint16_t *)L.src, (uint16_t *)L.out);
}
