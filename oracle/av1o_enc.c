/* av1o_enc.c - oracle key-frame encoder: bitstream syntax + closed-loop reconstruction.
 *
 * Boundary restated: one call = one frame of one scene-chunk, i.e. the unit of work the
 * reference hands to an external SVT-AV1 worker via av1an (`run_av1an`,
 * /root/reference/crates/daemon/src/encode/av1an.rs:126-139; operating point string
 * av1an.rs:14, here CQ=30 <-> base_q_idx 120).
 *
 * Normative syntax mirrored (AV1 spec section numbers):
 *   §5.3 OBU header, §5.5 sequence_header_obu, §5.9 uncompressed_header (key frame),
 *   §5.9.15 tile_info, §5.9.12 quantization_params, §5.9.11 loop_filter_params (levels 0),
 *   §5.9.19 cdef_params, §5.9.21 read_tx_mode (TX_MODE_LARGEST), §5.11.1 tile_group_obu,
 *   §5.11.4 decode_partition, §5.11.5 decode_block, §5.11.7 intra_frame_mode_info,
 *   §5.11.34 residual, §5.11.35 transform_block, §5.11.39 coeffs, §5.11.47 transform_type;
 *   context derivations §8.3.2; dequant §7.12.3; prediction edges §7.11.2.
 * Encoder decisions (non-normative, defined by this build): block size,
 * intra mode by SAD of the closed-loop prediction, tx type by mode, dead-zone quantiser.
 * Oracle code (test infrastructure): see av1o.h.
 */
#include "av1o.h"
#include "../av1-base_amd/csrc/av1_tables.h"
#include <stdlib.h>
#include <string.h>
#include <stdio.h>

/* ------------------------------------------------------------------ bit writer (headers) */
typedef struct {
  uint8_t *buf;
  size_t cap, pos; /* pos in bits */
} BitW;

static void bw_put(BitW *b, uint32_t v, int n) {
  int i;
  for (i = n - 1; i >= 0; i--) {
    size_t byte = b->pos >> 3;
    if (byte < b->cap) {
      if ((b->pos & 7) == 0) b->buf[byte] = 0;
      b->buf[byte] |= (uint8_t)(((v >> i) & 1) << (7 - (b->pos & 7)));
    }
    b->pos++;
  }
}
static void bw_trailing(BitW *b) {
  bw_put(b, 1, 1);
  while (b->pos & 7) bw_put(b, 0, 1);
}
static void bw_align(BitW *b) {
  while (b->pos & 7) bw_put(b, 0, 1);
}
static int leb128_size(uint64_t v) {
  int n = 1;
  while (v >>= 7) n++;
  return n;
}
static size_t put_leb128(uint8_t *p, uint64_t v) {
  size_t n = 0;
  do {
    uint8_t b = v & 0x7F;
    v >>= 7;
    if (v) b |= 0x80;
    p[n++] = b;
  } while (v);
  return n;
}
static int floor_log2(unsigned v) { return 31 - __builtin_clz(v); }
static int tile_log2(int blk, int target) {
  int k = 0;
  while ((blk << k) < target) k++;
  return k;
}
/* ns(n) non-symmetric unsigned (spec §4.10.7) */
static void bw_put_ns(BitW *b, int n, int v) {
  int w = floor_log2((unsigned)n) + 1;
  int m = (1 << w) - n;
  if (v < m) bw_put(b, (uint32_t)v, w - 1);
  else {
    int extra = v + m;
    bw_put(b, (uint32_t)(extra >> 1), w - 1);
    bw_put(b, (uint32_t)(extra & 1), 1);
  }
}

void av1o_default_config(Av1oConfig *c, int w, int h, int bit_depth) {
  memset(c, 0, sizeof(*c));
  c->width = w;
  c->height = h;
  c->bit_depth = bit_depth;
  c->base_q_idx = 120;
  c->tile_w_sb = 1;
  c->tile_h_sb = 1;
  c->min_bs_log2 = 4;
  c->max_bs_log2 = 4;
  c->enable_cdef = 1;
  c->cdef_y_pri = 2;
  c->cdef_y_sec = 0;
  c->cdef_uv_pri = 1;
  c->cdef_uv_sec = 0;
  c->cdef_damping = 5;
  c->mode_mask = 0x0007; /* DC, V, H */
  c->me_range = 8;
  c->subpel = 0;
  c->enable_qm = 0;
  c->qm_y = c->qm_uv = 15;
  c->fuzz_density = 8;
  c->fuzz_maxlevel = 40;
}

Av1oFrame *av1o_frame_alloc(int w, int h) {
  Av1oFrame *f = (Av1oFrame *)calloc(1, sizeof(*f));
  int p;
  f->w = w;
  f->h = h;
  for (p = 0; p < 3; p++) {
    int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
    f->stride[p] = pw;
    f->p[p] = (uint16_t *)calloc((size_t)pw * ph, sizeof(uint16_t));
  }
  return f;
}
void av1o_frame_free(Av1oFrame *f) {
  if (!f) return;
  free(f->p[0]);
  free(f->p[1]);
  free(f->p[2]);
  free(f);
}

/* frame size as signalled (and as the decoder crops / clamps references / restores): the true size when the encoder
 * runs on a source padded to multiples of 8 */
static int true_w(const Av1oConfig *cfg) { return cfg->true_width ? cfg->true_width : cfg->width; }
static int true_h(const Av1oConfig *cfg) { return cfg->true_height ? cfg->true_height : cfg->height; }

/* ------------------------------------------------------------------ sequence header §5.5 */
static void write_color_config(BitW *b, const Av1oConfig *cfg) {
  bw_put(b, cfg->bit_depth > 8, 1); /* high_bitdepth (profile 0: no twelve_bit) */
  bw_put(b, 0, 1);                  /* mono_chrome */
  {
    const int desc = cfg->color_primaries || cfg->transfer_characteristics || cfg->matrix_coefficients;
    bw_put(b, desc, 1);             /* color_description_present_flag */
    if (desc) { /* a field left at 0 is written as 2 "unspecified": MC 0 (identity) is not allowed with 4:2:0 (spec 5.5.2) */
      bw_put(b, (unsigned)(cfg->color_primaries ? cfg->color_primaries : 2), 8);
      bw_put(b, (unsigned)(cfg->transfer_characteristics ? cfg->transfer_characteristics : 2), 8);
      bw_put(b, (unsigned)(cfg->matrix_coefficients ? cfg->matrix_coefficients : 2), 8);
    }
    /* (CP 1 / TC 13 / MC 0 - sRGB with the identity matrix - would imply 4:4:4 and no color_range bit: not a 4:2:0 description,
     * refused by the product's parameter check, never written here) */
  }
  bw_put(b, cfg->color_range ? 1 : 0, 1); /* color_range: 0 studio (limited), 1 full */
  bw_put(b, 0, 2);                  /* chroma_sample_position (4:2:0): unknown */
  bw_put(b, 0, 1);                  /* separate_uv_delta_q */
}

static size_t seq_header_payload(const Av1oConfig *cfg, uint8_t *buf, size_t cap) {
  BitW b = { buf, cap, 0 };
  int wbits = floor_log2((unsigned)(true_w(cfg) - 1) | 1) + 1, hbits = floor_log2((unsigned)(true_h(cfg) - 1) | 1) + 1;
  bw_put(&b, 0, 3);                   /* seq_profile */
  bw_put(&b, cfg->still_picture, 1);  /* still_picture */
  bw_put(&b, cfg->still_picture, 1);  /* reduced_still_picture_header */
  if (cfg->still_picture) {
    bw_put(&b, 31, 5);                /* seq_level_idx[0] */
  } else {
    bw_put(&b, 0, 1);  /* timing_info_present_flag */
    bw_put(&b, 0, 1);  /* initial_display_delay_present_flag */
    bw_put(&b, 0, 5);  /* operating_points_cnt_minus_1 */
    bw_put(&b, 0, 12); /* operating_point_idc[0] */
    bw_put(&b, 31, 5); /* seq_level_idx[0] = 31 (maximum parameters) */
    bw_put(&b, 0, 1);  /* seq_tier[0] (present because level > 7) */
  }
  bw_put(&b, (uint32_t)(wbits - 1), 4);
  bw_put(&b, (uint32_t)(hbits - 1), 4);
  bw_put(&b, (uint32_t)(true_w(cfg) - 1), wbits);
  bw_put(&b, (uint32_t)(true_h(cfg) - 1), hbits);
  if (!cfg->still_picture) bw_put(&b, 0, 1); /* frame_id_numbers_present_flag */
  bw_put(&b, 0, 1); /* use_128x128_superblock */
  bw_put(&b, 0, 1); /* enable_filter_intra */
  bw_put(&b, cfg->intra_edge_filter ? 1 : 0, 1); /* enable_intra_edge_filter */
  if (!cfg->still_picture) {
    bw_put(&b, 0, 1); /* enable_interintra_compound */
    bw_put(&b, 0, 1); /* enable_masked_compound */
    bw_put(&b, 0, 1); /* enable_warped_motion */
    bw_put(&b, 0, 1); /* enable_dual_filter */
    bw_put(&b, 0, 1); /* enable_order_hint */
    bw_put(&b, 0, 1); /* seq_choose_screen_content_tools */
    bw_put(&b, 0, 1); /* seq_force_screen_content_tools = 0 */
  }
  bw_put(&b, 0, 1);               /* enable_superres */
  bw_put(&b, cfg->enable_cdef, 1); /* enable_cdef */
  bw_put(&b, (uint32_t)(cfg->enable_lr != 0), 1); /* enable_restoration */
  write_color_config(&b, cfg);
  bw_put(&b, (uint32_t)(cfg->film_grain != 0), 1); /* film_grain_params_present */
  bw_trailing(&b);
  return b.pos >> 3;
}

long av1o_write_sequence_header(const Av1oConfig *cfg, uint8_t *out, size_t cap) {
  uint8_t tmp[64];
  size_t n = seq_header_payload(cfg, tmp, sizeof(tmp)), k;
  if (cap < n + 3) return -1;
  out[0] = (1 << 3) | 2; /* OBU_SEQUENCE_HEADER, has_size_field */
  k = put_leb128(out + 1, n);
  memcpy(out + 1 + k, tmp, n);
  return (long)(1 + k + n);
}

/* ------------------------------------------------------------------ tile geometry */
typedef struct {
  int mi_rows, mi_cols, sb_rows, sb_cols;
  int tile_cols, tile_rows;
  int col_start_sb[65], row_start_sb[65];
} Geom;

static void make_geom(const Av1oConfig *cfg, Geom *g) {
  int i, s;
  g->mi_rows = cfg->height / 4;
  g->mi_cols = cfg->width / 4;
  g->sb_rows = (g->mi_rows + 15) >> 4;
  g->sb_cols = (g->mi_cols + 15) >> 4;
  for (i = 0, s = 0; s < g->sb_cols; i++, s += cfg->tile_w_sb) g->col_start_sb[i] = s;
  g->tile_cols = i;
  g->col_start_sb[i] = g->sb_cols;
  for (i = 0, s = 0; s < g->sb_rows; i++, s += cfg->tile_h_sb) g->row_start_sb[i] = s;
  g->tile_rows = i;
  g->row_start_sb[i] = g->sb_rows;
}

/* ------------------------------------------------------------------ frame header §5.9 */
#define TILE_SIZE_BYTES 4

static size_t frame_header_bits(const Av1oConfig *cfg, const Geom *g, int is_inter, uint8_t *buf, size_t cap) {
  BitW b = { buf, cap, 0 };
  int i;
  if (!cfg->still_picture) {
    bw_put(&b, 0, 1); /* show_existing_frame */
    bw_put(&b, is_inter ? 1 : 0, 2); /* frame_type = KEY_FRAME / INTER_FRAME */
    bw_put(&b, 1, 1); /* show_frame */
    /* error_resilient_mode = 1 implied for a shown key frame */
    if (is_inter) bw_put(&b, 0, 1); /* error_resilient_mode */
  }
  bw_put(&b, (uint32_t)cfg->disable_cdf_update, 1); /* disable_cdf_update */
  /* allow_screen_content_tools = seq_force_screen_content_tools = 0 (still: SELECT -> coded) */
  if (cfg->still_picture) bw_put(&b, 0, 1); /* allow_screen_content_tools */
  if (!cfg->still_picture) bw_put(&b, 0, 1); /* frame_size_override_flag */
  /* order_hint: 0 bits (enable_order_hint = 0) */
  if (is_inter) {
    bw_put(&b, 7, 3);    /* primary_ref_frame = PRIMARY_REF_NONE: every frame starts from the default CDFs */
    bw_put(&b, 0x01, 8); /* refresh_frame_flags: this frame replaces slot 0 */
    /* frame_refs_short_signaling = 0 (no order hints) */
    for (i = 0; i < 7; i++) bw_put(&b, 0, 3); /* ref_frame_idx[i] = 0: every reference name -> the previous frame */
  }
  /* key frame: primary_ref_frame = NONE, refresh_frame_flags = 0xFF implied */
  /* frame_size(): from sequence; superres_params(): none */
  bw_put(&b, 0, 1); /* render_and_frame_size_different */
  /* allow_intrabc not coded (allow_screen_content_tools = 0) */
  if (is_inter) {
    bw_put(&b, 0, 1); /* allow_high_precision_mv */
    bw_put(&b, 0, 1); /* is_filter_switchable */
    bw_put(&b, cfg->subpel ? 0 : 3, 2); /* interpolation_filter: EIGHTTAP (0) with sub-sample vectors, else BILINEAR (3) */
    bw_put(&b, 0, 1); /* is_motion_mode_switchable */
    /* use_ref_frame_mvs: not coded (enable_ref_frame_mvs = 0) */
  }
  if (!cfg->still_picture && !cfg->disable_cdf_update) bw_put(&b, 1, 1); /* disable_frame_end_update_cdf */
  /* tile_info() */
  {
    int sb_cols = g->sb_cols, sb_rows = g->sb_rows;
    int max_tile_width_sb = 4096 >> 6, max_tile_area_sb = (4096 * 2304) >> 12;
    int min_log2_tile_cols = tile_log2(max_tile_width_sb, sb_cols);
    int min_log2_tiles = tile_log2(max_tile_area_sb, sb_rows * sb_cols);
    int start, widest = 0, max_tile_height_sb, tile_cols_log2, tile_rows_log2;
    if (min_log2_tiles < min_log2_tile_cols) min_log2_tiles = min_log2_tile_cols;
    bw_put(&b, 0, 1); /* uniform_tile_spacing_flag = 0 */
    for (i = 0, start = 0; start < sb_cols; i++) {
      int max_w = sb_cols - start < max_tile_width_sb ? sb_cols - start : max_tile_width_sb;
      int sz = g->col_start_sb[i + 1] - g->col_start_sb[i];
      bw_put_ns(&b, max_w, sz - 1);
      if (sz > widest) widest = sz;
      start += sz;
    }
    {
      int area = sb_rows * sb_cols;
      if (min_log2_tiles > 0) area >>= (min_log2_tiles + 1);
      max_tile_height_sb = area / widest;
      if (max_tile_height_sb < 1) max_tile_height_sb = 1;
    }
    for (i = 0, start = 0; start < sb_rows; i++) {
      int max_h = sb_rows - start < max_tile_height_sb ? sb_rows - start : max_tile_height_sb;
      int sz = g->row_start_sb[i + 1] - g->row_start_sb[i];
      bw_put_ns(&b, max_h, sz - 1);
      start += sz;
    }
    tile_cols_log2 = tile_log2(1, g->tile_cols);
    tile_rows_log2 = tile_log2(1, g->tile_rows);
    if (tile_cols_log2 > 0 || tile_rows_log2 > 0) {
      bw_put(&b, 0, tile_cols_log2 + tile_rows_log2); /* context_update_tile_id */
      bw_put(&b, TILE_SIZE_BYTES - 1, 2);              /* tile_size_bytes_minus_1 */
    }
  }
  /* quantization_params() */
  bw_put(&b, (uint32_t)cfg->base_q_idx, 8);
  bw_put(&b, 0, 1); /* DeltaQYDc delta_coded */
  bw_put(&b, 0, 1); /* DeltaQUDc */
  bw_put(&b, 0, 1); /* DeltaQUAc */
  bw_put(&b, cfg->enable_qm ? 1 : 0, 1); /* using_qmatrix */
  if (cfg->enable_qm) {
    bw_put(&b, (uint32_t)cfg->qm_y, 4);  /* qm_y */
    bw_put(&b, (uint32_t)cfg->qm_uv, 4); /* qm_u; qm_v = qm_u because separate_uv_delta_q = 0 */
  }
  bw_put(&b, 0, 1); /* segmentation_enabled */
  if (cfg->base_q_idx > 0) bw_put(&b, 0, 1); /* delta_q_present */
  /* loop_filter_params() §5.9.11: levels 0 = deblocking off */
  {
    int lv[4];
    av1o_deblock_levels(cfg, !is_inter, lv);
    bw_put(&b, (uint32_t)lv[0], 6);
    bw_put(&b, (uint32_t)lv[1], 6);
    if (lv[0] || lv[1]) { bw_put(&b, (uint32_t)lv[2], 6); bw_put(&b, (uint32_t)lv[3], 6); }
    bw_put(&b, (uint32_t)(cfg->deblock == 2 ? cfg->lf_sharpness : 0), 3); /* loop_filter_sharpness */
    bw_put(&b, 0, 1); /* loop_filter_delta_enabled */
  }
  /* cdef_params() */
  if (cfg->enable_cdef) {
    bw_put(&b, (uint32_t)(cfg->cdef_damping - 3), 2);
    bw_put(&b, 0, 2); /* cdef_bits */
    bw_put(&b, (uint32_t)cfg->cdef_y_pri, 4);
    bw_put(&b, (uint32_t)cfg->cdef_y_sec, 2);
    bw_put(&b, (uint32_t)cfg->cdef_uv_pri, 4);
    bw_put(&b, (uint32_t)cfg->cdef_uv_sec, 2);
  }
  if (cfg->enable_lr) { /* lr_params() §5.9.20: luma RESTORE_WIENER (lr_type 2), chroma RESTORE_NONE, 64x64 units */
    bw_put(&b, cfg->enable_lr == 2 ? 1 : 2, 2); /* lr_type: 1 -> RESTORE_SWITCHABLE, 2 -> RESTORE_WIENER */
    bw_put(&b, 0, 2);
    bw_put(&b, 0, 2);
    bw_put(&b, 0, 1); /* lr_unit_shift = 0: LoopRestorationSize = 256 >> 2 = 64 (no lr_uv_shift: chroma unused) */
  }
  bw_put(&b, 0, 1); /* tx_mode_select = 0 -> TX_MODE_LARGEST */
  if (is_inter) bw_put(&b, 0, 1); /* reference_select = 0: single reference */
  /* skip_mode_present: not coded (no order hints); allow_warped_motion: not coded (enable_warped_motion = 0) */
  bw_put(&b, 0, 1); /* reduced_tx_set */
  if (is_inter)
    for (i = 0; i < 7; i++) bw_put(&b, 0, 1); /* global_motion_params: is_global = 0 for LAST..ALTREF */
  if (cfg->film_grain) { /* film_grain_params() §5.9.30 (show_frame = 1) */
    int pl;
    bw_put(&b, 1, 1);                                   /* apply_grain */
    bw_put(&b, (uint32_t)cfg->fg_seed & 0xFFFF, 16);    /* grain_seed */
    if (is_inter) bw_put(&b, 1, 1);                     /* update_grain (implied 1 on key frames) */
    bw_put(&b, 2, 4);                                   /* num_y_points */
    bw_put(&b, 0, 8);   bw_put(&b, (uint32_t)cfg->fg_y_scaling, 8);
    bw_put(&b, 255, 8); bw_put(&b, (uint32_t)cfg->fg_y_scaling, 8);
    bw_put(&b, 0, 1);                                   /* chroma_scaling_from_luma */
    for (pl = 0; pl < 2; pl++) {                        /* num_cb_points, num_cr_points */
      bw_put(&b, 2, 4);
      bw_put(&b, 0, 8);   bw_put(&b, (uint32_t)cfg->fg_c_scaling, 8);
      bw_put(&b, 255, 8); bw_put(&b, (uint32_t)cfg->fg_c_scaling, 8);
    }
    bw_put(&b, 3, 2);                                   /* grain_scaling_minus_8 */
    bw_put(&b, 0, 2);                                   /* ar_coeff_lag: numPosLuma = 0, numPosChroma = 1 */
    bw_put(&b, 128, 8);                                 /* ar_coeffs_cb_plus_128[0] (luma coupling 0) */
    bw_put(&b, 128, 8);                                 /* ar_coeffs_cr_plus_128[0] */
    bw_put(&b, 0, 2);                                   /* ar_coeff_shift_minus_6 */
    bw_put(&b, 0, 2);                                   /* grain_scale_shift */
    for (pl = 0; pl < 2; pl++) {
      bw_put(&b, 128, 8);                               /* cb/cr_mult */
      bw_put(&b, 192, 8);                               /* cb/cr_luma_mult */
      bw_put(&b, 256, 9);                               /* cb/cr_offset */
    }
    bw_put(&b, 1, 1);                                   /* overlap_flag */
    bw_put(&b, 0, 1);                                   /* clip_to_restricted_range */
  }
  return b.pos;
}

/* ------------------------------------------------------------------ per-tile coding state */
typedef struct {
  uint16_t partition[20][11];
  uint16_t kf_y_mode[5][5][14];
  uint16_t uv_mode[2][13][15];
  uint16_t cfl_sign[9], cfl_alpha[6][17];
  uint16_t angle_delta[8][8];
  uint16_t skip[3][3];
  uint16_t intra_tx_set1[2][13][8];
  uint16_t intra_tx_set2[3][13][6];
  uint16_t txb_skip[5][13][3];
  uint16_t eob_pt_16[2][2][6], eob_pt_32[2][2][7], eob_pt_64[2][2][8], eob_pt_128[2][2][9];
  uint16_t eob_pt_256[2][2][10], eob_pt_512[2][2][11], eob_pt_1024[2][2][12];
  uint16_t eob_extra[5][2][9][3];
  uint16_t dc_sign[2][3][3];
  uint16_t coeff_base_eob[5][2][4][4];
  uint16_t coeff_base[5][2][42][5];
  uint16_t coeff_br[5][2][21][5];
  /* inter frames */
  uint16_t y_mode[4][14];
  uint16_t is_inter[4][3];
  uint16_t newmv[6][3], globalmv[2][3], refmv[6][3], drl[3][3];
  uint16_t single_ref[6][3][3]; /* [p1..p6][ctx] */
  uint16_t inter_tx_set1[2][17], inter_tx_set2[13], inter_tx_set3[4][3];
  uint16_t mv_joint[5];
  uint16_t use_wiener[3];
  uint16_t restoration_type[4];
  struct {
    uint16_t cls[12], class0_fp[2][5], fp[5], sign[3], class0_hp[3], hp[3], class0[3], bits[10][3];
  } mvc[2];
} TileCdfs;

static void load_cdf(uint16_t *dst, const uint16_t *src, int nsym) {
  int i;
  for (i = 0; i < nsym - 1; i++) dst[i] = (uint16_t)(32768 - src[i]);
  dst[nsym - 1] = 0;
  dst[nsym] = 0;
}

static void init_cdfs(TileCdfs *c, int qidx) {
  int q = qidx <= 20 ? 0 : (qidx <= 60 ? 1 : (qidx <= 120 ? 2 : 3));
  int i, j, k, l;
  for (i = 0; i < 20; i++) load_cdf(c->partition[i], av1_default_partition_cdf[i], i < 4 ? 4 : (i < 16 ? 10 : 8));
  for (i = 0; i < 5; i++)
    for (j = 0; j < 5; j++) load_cdf(c->kf_y_mode[i][j], av1_default_kf_y_mode_cdf[i][j], 13);
  for (i = 0; i < 13; i++) {
    load_cdf(c->uv_mode[0][i], av1_default_uv_mode_nocfl_cdf[i], 13);
    load_cdf(c->uv_mode[1][i], av1_default_uv_mode_cfl_cdf[i], 14);
  }
  load_cdf(c->cfl_sign, av1_default_cfl_sign_cdf[0], 8);
  for (i = 0; i < 6; i++) load_cdf(c->cfl_alpha[i], av1_default_cfl_alpha_cdf[i], 16);
  for (i = 0; i < 8; i++) load_cdf(c->angle_delta[i], av1_default_angle_delta_cdf[i], 7);
  for (i = 0; i < 3; i++) load_cdf(c->skip[i], av1_default_skip_cdf[i], 2);
  for (i = 0; i < 2; i++)
    for (j = 0; j < 13; j++) load_cdf(c->intra_tx_set1[i][j], av1_default_intra_tx_set1_cdf[i][j], 7);
  for (i = 0; i < 3; i++)
    for (j = 0; j < 13; j++) load_cdf(c->intra_tx_set2[i][j], av1_default_intra_tx_set2_cdf[i][j], 5);
  for (i = 0; i < 5; i++)
    for (j = 0; j < 13; j++) load_cdf(c->txb_skip[i][j], av1_default_txb_skip_cdf[q][i][j], 2);
  for (i = 0; i < 2; i++)
    for (j = 0; j < 2; j++) {
      load_cdf(c->eob_pt_16[i][j], av1_default_eob_multi16_cdf[q][i][j], 5);
      load_cdf(c->eob_pt_32[i][j], av1_default_eob_multi32_cdf[q][i][j], 6);
      load_cdf(c->eob_pt_64[i][j], av1_default_eob_multi64_cdf[q][i][j], 7);
      load_cdf(c->eob_pt_128[i][j], av1_default_eob_multi128_cdf[q][i][j], 8);
      load_cdf(c->eob_pt_256[i][j], av1_default_eob_multi256_cdf[q][i][j], 9);
      load_cdf(c->eob_pt_512[i][j], av1_default_eob_multi512_cdf[q][i][j], 10);
      load_cdf(c->eob_pt_1024[i][j], av1_default_eob_multi1024_cdf[q][i][j], 11);
    }
  for (i = 0; i < 5; i++)
    for (j = 0; j < 2; j++) {
      for (k = 0; k < 9; k++) load_cdf(c->eob_extra[i][j][k], av1_default_eob_extra_cdf[q][i][j][k], 2);
      for (k = 0; k < 4; k++) load_cdf(c->coeff_base_eob[i][j][k], av1_default_coeff_base_eob_cdf[q][i][j][k], 3);
      for (k = 0; k < 42; k++) load_cdf(c->coeff_base[i][j][k], av1_default_coeff_base_cdf[q][i][j][k], 4);
      for (k = 0; k < 21; k++) load_cdf(c->coeff_br[i][j][k], av1_default_coeff_br_cdf[q][i][j][k], 4);
    }
  for (j = 0; j < 2; j++)
    for (l = 0; l < 3; l++) load_cdf(c->dc_sign[j][l], av1_default_dc_sign_cdf[q][j][l], 2);
  /* inter frames */
  for (i = 0; i < 4; i++) {
    load_cdf(c->y_mode[i], av1_default_if_y_mode_cdf[i], 13);
    load_cdf(c->is_inter[i], av1_default_is_inter_cdf[i], 2);
    load_cdf(c->inter_tx_set3[i], av1_default_inter_tx_set3_cdf[i], 2);
  }
  for (i = 0; i < 6; i++) {
    load_cdf(c->newmv[i], av1_default_newmv_cdf[i], 2);
    load_cdf(c->refmv[i], av1_default_refmv_cdf[i], 2);
    for (j = 0; j < 3; j++) load_cdf(c->single_ref[i][j], av1_default_single_ref_cdf[i][j], 2);
  }
  for (i = 0; i < 2; i++) load_cdf(c->globalmv[i], av1_default_globalmv_cdf[i], 2);
  for (i = 0; i < 3; i++) load_cdf(c->drl[i], av1_default_drl_cdf[i], 2);
  for (i = 0; i < 2; i++) load_cdf(c->inter_tx_set1[i], av1_default_inter_tx_set1_cdf[i], 16);
  load_cdf(c->inter_tx_set2, av1_default_inter_tx_set2_cdf[0], 12);
  load_cdf(c->mv_joint, av1_default_mv_joint_cdf[0], 4);
  load_cdf(c->use_wiener, av1_default_use_wiener_cdf[0], 2);
  load_cdf(c->restoration_type, av1_default_switchable_restore_cdf[0], 3);
  for (i = 0; i < 2; i++) {
    load_cdf(c->mvc[i].cls, av1_default_mv_class_cdf[0], 11);
    for (j = 0; j < 2; j++) load_cdf(c->mvc[i].class0_fp[j], av1_default_mv_class0_fp_cdf[j], 4);
    load_cdf(c->mvc[i].fp, av1_default_mv_fp_cdf[0], 4);
    load_cdf(c->mvc[i].sign, av1_default_mv_sign_cdf[0], 2);
    load_cdf(c->mvc[i].class0_hp, av1_default_mv_class0_hp_cdf[0], 2);
    load_cdf(c->mvc[i].hp, av1_default_mv_hp_cdf[0], 2);
    load_cdf(c->mvc[i].class0, av1_default_mv_class0_cdf[0], 2);
    for (j = 0; j < 10; j++) load_cdf(c->mvc[i].bits[j], av1_default_mv_bits_cdf[j], 2);
  }
}

typedef struct Enc_ {
  const Av1oConfig *cfg;
  const Geom *g;
  const Av1oFrame *src;
  Av1oFrame *rec;      /* pre-CDEF reconstruction */
  /* frame-level per-mi maps */
  uint8_t *mi_bsl;     /* log2 of block size in pixels of the block covering the mi, 0 = not coded */
  uint8_t *mi_skip;
  uint8_t *mi_ymode;
  uint8_t *mi_uvmode;  /* get_filter_type() of chroma blocks (spec 7.11.2.8) */
  /* inter frames */
  const Av1oFrame *ref; /* LAST_FRAME: the previous frame's final reconstruction; NULL on key frames */
  const Av1oFrame *prev_src; /* the previous SOURCE frame: what the motion search looks at */
  int16_t *me_centre;   /* cfg->me_presearch: per superblock {row, col} of the full search's centre, whole luma samples (multiples of 8) */
  uint8_t *mi_is_inter; /* 1: block predicted from LAST_FRAME */
  uint8_t *mi_newmv;    /* 1: coded as NEWMV (counts towards NewMvCount of later blocks) */
  int16_t *mi_mv;       /* [mi][2] = {row, col} in 1/8 luma samples */
  /* loop restoration: unit decisions of this frame (NULL while they are not known yet: first pass) */
  const Av1oLrUnit *lr_units;
  int ref_lr[2][3];     /* RefLrWiener[0][pass][tap], reset per tile */
  int ref_sgr[2];       /* RefSgrXqd[0][i], reset per tile */
  int8_t *cdef_idx_sb;
  /* tile state */
  int mi_row_start, mi_row_end, mi_col_start, mi_col_end;
  TileCdfs cdf;
  Av1oRangeEnc ec;
  uint8_t *above_lvl[3], *above_dc[3]; /* indexed by absolute 4x4 column of the plane */
  uint8_t left_lvl[3][16], left_dc[3][16]; /* indexed by 4x4 row within the SB (plane units) */
  uint8_t block_decoded[3][19][19];    /* [plane][y+1][x+1], y,x in -1..17 (plane 4x4 units in SB) */
  int dc_q, ac_q;
  Av1oStats *stats;
  uint32_t rng_state;
} Enc;

static uint32_t fuzz_rand(Enc *e) {
  /* xorshift32 */
  uint32_t x = e->rng_state;
  x ^= x << 13;
  x ^= x >> 17;
  x ^= x << 5;
  e->rng_state = x;
  return x;
}

/* ------------------------------------------------------------------ tables */
static const uint8_t intra_mode_context[13] = { 0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0 };
static const uint8_t mode_to_txfm[14] = { DCT_DCT, ADST_DCT, DCT_ADST, DCT_DCT, ADST_ADST, ADST_DCT, DCT_ADST,
                                          DCT_ADST, ADST_DCT, ADST_ADST, ADST_DCT, DCT_ADST, ADST_ADST, DCT_DCT };
/* symbol index of a tx type inside the intra sets (Tx_Type_Intra_Inv_Set1/2 inverted) */
static int tx_type_to_sym(int set, int tx_type) {
  static const int8_t s1[16] = { 1, 5, 6, 4, -1, -1, -1, -1, -1, 0, 2, 3, -1, -1, -1, -1 };
  static const int8_t s2[16] = { 1, 3, 4, 2, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1 };
  return set == 1 ? s1[tx_type] : s2[tx_type];
}
/* Coeff_Base_Ctx_Offset for square transforms (spec §8.3.2 table) */
static int coeff_base_ctx_offset(int log2n, int row, int col) {
  static const uint8_t off[5][5] = { { 0, 1, 6, 6, 21 }, { 1, 6, 6, 21, 21 }, { 6, 6, 21, 21, 21 }, { 6, 21, 21, 21, 21 }, { 21, 21, 21, 21, 21 } };
  (void)log2n;
  if (row > 4) row = 4;
  if (col > 4) col = 4;
  return off[row][col];
}

static void write_sym(struct Enc_ *e, int s, uint16_t *icdf, int n);
static int is_inside(const Enc *e, int r, int c) {
  return c >= e->mi_col_start && c < e->mi_col_end && r >= e->mi_row_start && r < e->mi_row_end;
}

#define WRITE_SYM(e, s, cdf, n) write_sym((e), (s), (cdf), (n))

static void write_sym(Enc *e, int s, uint16_t *icdf, int n) {
  if (e->cfg->disable_cdf_update) {
    uint16_t tmp[17];
    memcpy(tmp, icdf, sizeof(uint16_t) * (size_t)(n + 1));
    av1o_ec_encode_symbol(&e->ec, s, tmp, n);
  } else {
    av1o_ec_encode_symbol(&e->ec, s, icdf, n);
  }
}

/* ------------------------------------------------------------------ coefficient coding §5.11.39 */
typedef struct {
  int32_t level[1024]; /* signed quantised levels, row-major in the (<=32)x(<=32) coded area */
  int eob;
  int tx_type;
} TxbCoefs;

static void write_golomb(Enc *e, unsigned x) {
  /* x >= 0; codes x+1 as in read_golomb (spec §5.11.39) */
  unsigned v = x + 1;
  int len = floor_log2(v) + 1, i;
  for (i = 0; i < len - 1; i++) av1o_ec_encode_literal(&e->ec, 0, 1);
  for (i = len - 1; i >= 0; i--) av1o_ec_encode_literal(&e->ec, (v >> i) & 1, 1);
}

static void write_coeffs(Enc *e, int plane, int log2n, int x4, int y4_sb, int y4_abs, const TxbCoefs *t, int ymode, int bw_eq_tx, int is_inter) {
  /* x4: absolute 4x4 column (plane units); y4_sb: 4x4 row within SB (plane units) */
  const int ptype = plane > 0;
  const int txs_ctx = log2n - 2; /* square: (sqr + sqr_up + 1) >> 1 */
  const int n = 1 << log2n, w4 = n >> 2;
  const int bwl = log2n > 5 ? 5 : log2n; /* coded area is at most 32x32 */
  const int cw = 1 << bwl;
  const int max_x4 = plane ? e->g->mi_cols >> 1 : e->g->mi_cols;
  const int max_y4 = plane ? e->g->mi_rows >> 1 : e->g->mi_rows;
  int k, ctx, c;
  TileCdfs *cdf = &e->cdf;
  const int16_t *scan = av1o_default_scan(bwl);
  /* --- all_zero (txb_skip) context */
  if (plane == 0) {
    int top = 0, left = 0;
    for (k = 0; k < w4; k++) {
      if (x4 + k < max_x4 && e->above_lvl[0][x4 + k] > top) top = e->above_lvl[0][x4 + k];
      if (y4_abs + k < max_y4 && e->left_lvl[0][y4_sb + k] > left) left = e->left_lvl[0][y4_sb + k];
    }
    if (bw_eq_tx) ctx = 0;
    else if (top == 0 && left == 0) ctx = 1;
    else if (top == 0 || left == 0) ctx = 2 + ((top > left ? top : left) > 3);
    else if ((top > left ? top : left) <= 3) ctx = 4;
    else if ((top < left ? top : left) <= 3) ctx = 5;
    else ctx = 6;
  } else {
    int above = 0, left = 0;
    for (k = 0; k < w4; k++) {
      if (x4 + k < max_x4) above |= e->above_lvl[plane][x4 + k] | e->above_dc[plane][x4 + k];
      if (y4_abs + k < max_y4) left |= e->left_lvl[plane][y4_sb + k] | e->left_dc[plane][y4_sb + k];
    }
    ctx = 7 + (above != 0) + (left != 0);
    /* (+3 when the plane block is larger than the transform: never with TX_MODE_LARGEST squares) */
  }
  WRITE_SYM(e, t->eob == 0, cdf->txb_skip[txs_ctx][ctx], 2);
  if (t->eob == 0) {
    for (k = 0; k < w4; k++) {
      if (x4 + k < max_x4) { e->above_lvl[plane][x4 + k] = 0; e->above_dc[plane][x4 + k] = 0; }
      if (y4_abs + k < max_y4) { e->left_lvl[plane][y4_sb + k] = 0; e->left_dc[plane][y4_sb + k] = 0; }
    }
    return;
  }
  /* --- transform_type (luma only, sets with more than one type) */
  if (plane == 0 && is_inter && log2n <= 5 && e->cfg->base_q_idx > 0) {
    /* inter_tx_type: this build codes every inter block DCT_DCT.  Symbol of DCT_DCT in the inverse maps of
     * TX_SET_INTER_1 (16 types: 4x4, 8x8) = 7, TX_SET_INTER_2 (12 types: 16x16) = 3, TX_SET_INTER_3
     * ({IDTX, DCT_DCT}: 32x32) = 1 (spec §5.11.47, Tx_Type_Inter_Inv_Set1/2/3) */
    if (log2n <= 3) WRITE_SYM(e, 7, cdf->inter_tx_set1[log2n - 2], 16);
    else if (log2n == 4) WRITE_SYM(e, 3, cdf->inter_tx_set2, 12);
    else WRITE_SYM(e, 1, cdf->inter_tx_set3[3], 2);
  } else if (plane == 0 && log2n <= 4 && e->cfg->base_q_idx > 0) {
    if (log2n <= 3) WRITE_SYM(e, tx_type_to_sym(1, t->tx_type), cdf->intra_tx_set1[log2n - 2][ymode], 7);
    else WRITE_SYM(e, tx_type_to_sym(2, t->tx_type), cdf->intra_tx_set2[log2n - 2][ymode], 5);
  }
  /* --- eob */
  {
    int eob = t->eob;
    int eob_pt = eob <= 2 ? eob : floor_log2((unsigned)(eob - 1)) + 2;
    int base = eob_pt < 2 ? eob_pt : ((1 << (eob_pt - 2)) + 1);
    int extra = eob - base;
    int msz = 2 * bwl - 4; /* eobMultisize */
    int mctx = 0;          /* TX_CLASS_2D */
    switch (msz) {
      case 0: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_16[ptype][mctx], 5); break;
      case 1: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_32[ptype][mctx], 6); break;
      case 2: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_64[ptype][mctx], 7); break;
      case 3: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_128[ptype][mctx], 8); break;
      case 4: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_256[ptype][mctx], 9); break;
      case 5: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_512[ptype][mctx], 10); break;
      default: WRITE_SYM(e, eob_pt - 1, cdf->eob_pt_1024[ptype][mctx], 11); break;
    }
    if (eob_pt >= 3) {
      int nbits = eob_pt - 2, i;
      int bit = (extra >> (nbits - 1)) & 1;
      WRITE_SYM(e, bit, cdf->eob_extra[txs_ctx][ptype][eob_pt - 3], 2);
      for (i = 1; i < nbits; i++) av1o_ec_encode_literal(&e->ec, (unsigned)((extra >> (nbits - 1 - i)) & 1), 1);
    }
  }
  /* --- levels, reverse scan order */
  for (c = t->eob - 1; c >= 0; c--) {
    int pos = scan[c];
    int row = pos >> bwl, col = pos & (cw - 1);
    int level = abs(t->level[pos]);
#define LV(r_, c_) (((r_) < cw && (c_) < cw) ? abs(t->level[((r_) << bwl) + (c_)]) : 0)
    if (c == t->eob - 1) {
      int cctx = c == 0 ? 0 : (c <= (cw * cw) / 8 ? 1 : (c <= (cw * cw) / 4 ? 2 : 3));
      WRITE_SYM(e, (level > 3 ? 3 : level) - 1, cdf->coeff_base_eob[txs_ctx][ptype][cctx], 3);
    } else {
      int mag, cctx;
#define M3(v) ((v) > 3 ? 3 : (v))
      mag = M3(LV(row, col + 1)) + M3(LV(row + 1, col)) + M3(LV(row + 1, col + 1)) + M3(LV(row, col + 2)) + M3(LV(row + 2, col));
      if (row == 0 && col == 0) cctx = 0;
      else {
        cctx = (mag + 1) >> 1;
        if (cctx > 4) cctx = 4;
        cctx += coeff_base_ctx_offset(log2n, row, col);
      }
      WRITE_SYM(e, level > 3 ? 3 : level, cdf->coeff_base[txs_ctx][ptype][cctx], 4);
    }
    if (level > 2) {
      int mag, bctx, idx;
#define M15(v) ((v) > 15 ? 15 : (v))
      mag = M15(LV(row, col + 1)) + M15(LV(row + 1, col)) + M15(LV(row + 1, col + 1));
      mag = (mag + 1) >> 1;
      if (mag > 6) mag = 6;
      if (pos == 0) bctx = mag;
      else if (row < 2 && col < 2) bctx = mag + 7;
      else bctx = mag + 14;
      for (idx = 0; idx < 4; idx++) {
        int rem = level - 3 - idx * 3;
        int k3 = rem > 3 ? 3 : rem;
        WRITE_SYM(e, k3, cdf->coeff_br[txs_ctx > 3 ? 3 : txs_ctx][ptype][bctx], 4);
        if (k3 < 3) break;
      }
    }
  }
  /* --- signs + golomb, forward scan order; context bookkeeping */
  {
    int cul = 0, dc_cat = 0;
    for (c = 0; c < t->eob; c++) {
      int pos = scan[c];
      int v = t->level[pos], level = abs(v);
      if (!level) continue;
      if (c == 0) {
        int dsum = 0, dctx;
        for (k = 0; k < w4; k++) {
          if (x4 + k < max_x4) { int s = e->above_dc[plane][x4 + k]; dsum += s == 1 ? -1 : (s == 2 ? 1 : 0); }
          if (y4_abs + k < max_y4) { int s = e->left_dc[plane][y4_sb + k]; dsum += s == 1 ? -1 : (s == 2 ? 1 : 0); }
        }
        dctx = dsum < 0 ? 1 : (dsum > 0 ? 2 : 0);
        WRITE_SYM(e, v < 0, cdf->dc_sign[ptype][dctx], 2);
      } else {
        av1o_ec_encode_literal(&e->ec, v < 0, 1);
      }
      if (level > 14) write_golomb(e, (unsigned)(level - 15));
      cul += level;
      if (pos == 0) dc_cat = v < 0 ? 1 : 2;
    }
    if (cul > 63) cul = 63;
    for (k = 0; k < w4; k++) {
      if (x4 + k < max_x4) { e->above_lvl[plane][x4 + k] = (uint8_t)cul; e->above_dc[plane][x4 + k] = (uint8_t)dc_cat; }
      if (y4_abs + k < max_y4) { e->left_lvl[plane][y4_sb + k] = (uint8_t)cul; e->left_dc[plane][y4_sb + k] = (uint8_t)dc_cat; }
    }
  }
}

/* ------------------------------------------------------------------ prediction edges §7.11.2 */
static void prepare_edges(const Enc *e, int plane, int x, int y, int n, int have_left, int have_above,
                          int have_above_rt, int have_below_lft, uint16_t *above_m1, uint16_t *left_m1) {
  const uint16_t *f = e->rec->p[plane];
  const int stride = e->rec->stride[plane];
  const int bd = e->cfg->bit_depth;
  const int max_x = (plane ? e->cfg->width / 2 : e->cfg->width) - 1;
  const int max_y = (plane ? e->cfg->height / 2 : e->cfg->height) - 1;
  uint16_t *A = above_m1 + 1, *L = left_m1 + 1;
  int i;
  if (!have_above && have_left) {
    for (i = 0; i < 2 * n; i++) A[i] = f[y * stride + x - 1];
  } else if (!have_above && !have_left) {
    for (i = 0; i < 2 * n; i++) A[i] = (uint16_t)((1 << (bd - 1)) - 1);
  } else {
    int lim = x + (have_above_rt ? 2 * n : n) - 1;
    if (lim > max_x) lim = max_x;
    for (i = 0; i < 2 * n; i++) A[i] = f[(y - 1) * stride + (x + i < lim ? x + i : lim)];
  }
  if (!have_left && have_above) {
    for (i = 0; i < 2 * n; i++) L[i] = f[(y - 1) * stride + x];
  } else if (!have_left && !have_above) {
    for (i = 0; i < 2 * n; i++) L[i] = (uint16_t)((1 << (bd - 1)) + 1);
  } else {
    int lim = y + (have_below_lft ? 2 * n : n) - 1;
    if (lim > max_y) lim = max_y;
    for (i = 0; i < 2 * n; i++) L[i] = f[(y + i < lim ? y + i : lim) * stride + x - 1];
  }
  if (have_above && have_left) A[-1] = f[(y - 1) * stride + x - 1];
  else if (have_above) A[-1] = f[(y - 1) * stride + x];
  else if (have_left) A[-1] = f[y * stride + x - 1];
  else A[-1] = (uint16_t)(1 << (bd - 1));
  L[-1] = A[-1];
}

/* ------------------------------------------------------------------ quantiser */
static int tx_scale_shift(int log2n) { return log2n >= 6 ? 2 : (log2n == 5 ? 1 : 0); }

/* Quantiser-matrix level from the quantiser index, as SVT-AV1 and libaom derive it from "--qm-min" / "--qm-max"
 * (the reference runs `--enable-qm 1 --qm-min 1 --qm-max 15`, av1an.rs:14). */
int av1o_qm_level(int base_q_idx, int qm_min, int qm_max) { return qm_min + base_q_idx * (qm_max + 1 - qm_min) / 256; }

/* §7.12.3: the dequantiser step at coefficient (i, j): q, or with a quantiser matrix Round2(q * Quantizer_Matrix[..], 5).
 * The matrix applies to the 2-D DCT/ADST types (PlaneTxType < IDTX) whenever the plane's level is < 15. */
static uint32_t qstep_at(const Enc *e, int plane, int log2n, int i, int j, int tx_type) {
  static const int off[4] = { AV1_QM_4X4, AV1_QM_8X8, AV1_QM_16X16, AV1_QM_32X32 };
  const uint32_t q = (uint32_t)((i | j) ? e->ac_q : e->dc_q);
  const int lvl = e->cfg->enable_qm ? (plane ? e->cfg->qm_uv : e->cfg->qm_y) : 15;
  const int l2 = log2n > 5 ? 5 : log2n;
  if (lvl >= 15 || tx_type >= IDTX) return q;   /* §7.12.3: the matrix applies only when PlaneTxType < IDTX */
  return (q * av1_qm_iwt[lvl][plane > 0][off[l2 - 2] + (i << l2) + j] + 16) >> 5;
}

/* forward transform + dead-zone quantise -> levels; dequantise + inverse -> recon in place.
 * Returns eob.  DESIGN.md §3.5: level = ((|coef| << s) + rnd) * ceil(2^32/q) >> 32 with the
 * frequency-dependent dead zone rnd = 3q/8 (row+col < n/4), q/4 (< n/2), q/8 (else). */
static int code_tx_block(Enc *e, int plane, int x, int y, int log2n, int tx_type, TxbCoefs *t, int allow_idtx) {
  const int n = 1 << log2n, bd = e->cfg->bit_depth;
  const int cw = n > 32 ? 32 : n, bwl = log2n > 5 ? 5 : log2n;
  const int sh = tx_scale_shift(log2n);
  const uint16_t *src = e->src->p[plane] + (size_t)y * e->src->stride[plane] + x;
  uint16_t *rec = e->rec->p[plane] + (size_t)y * e->rec->stride[plane] + x;
  const int sstride = e->src->stride[plane], rstride = e->rec->stride[plane];
  int32_t *resid = (int32_t *)malloc(sizeof(int32_t) * n * n * 2);
  int32_t *coef = resid + n * n;
  const int16_t *scan = av1o_default_scan(bwl);
  int i, j, eob = 0, c;
  t->tx_type = tx_type;
  memset(t->level, 0, sizeof(int32_t) * cw * cw);
  for (i = 0; i < n; i++)
    for (j = 0; j < n; j++) resid[i * n + j] = (int32_t)src[i * sstride + j] - (int32_t)rec[i * rstride + j];
  /* transform type search (cfg->tx_search): an intra luma block of up to 16x16 whose residual is sparse - at
   * most one sample in eight is nonzero - is coded with the identity transform (IDTX): flat areas with isolated edges, text */
  if (allow_idtx) {
    int nnz = 0;
    for (c = 0; c < n * n; c++) nnz += resid[c] != 0;
    if (e->cfg->fuzz_modes) { if (fuzz_rand(e) % 3 == 0) tx_type = IDTX; }
    else if (nnz * 8 <= n * n) tx_type = IDTX;
    t->tx_type = tx_type;
  }
  if (e->cfg->fuzz_coeffs) {
    for (c = 0; c < cw * cw; c++) {
      if (fuzz_rand(e) % (unsigned)e->cfg->fuzz_density == 0) {
        int lv = 1 + (int)(fuzz_rand(e) % (unsigned)e->cfg->fuzz_maxlevel);
        if (fuzz_rand(e) & 1) lv = 1 + (lv & 1);
        t->level[scan[c]] = (fuzz_rand(e) & 1) ? -lv : lv;
      }
      if ((fuzz_rand(e) & 63) == 0) break; /* vary eob */
    }
  } else {
    /* luma 32x32 blocks: the forward transform is the exact-integer matrix product of DESIGN.md §3 item 3e (what the HIP path's matrix
     * cores compute); every other size and plane: the butterfly networks */
    if (plane == 0 && log2n == 5) av1o_fwd_dct32x32_matrix(resid, n, coef);
    else av1o_fwd_txfm2d(resid, n, coef, log2n, tx_type, bd);
    for (i = 0; i < cw; i++)
      for (j = 0; j < cw; j++) {
        int32_t v = coef[i * n + j];
        uint32_t q = qstep_at(e, plane, log2n, i, j, tx_type);
        uint32_t recip = (uint32_t)((((uint64_t)1 << 32) + q - 1) / q);
        uint32_t rnd = (i + j) < (cw >> 2) ? (3 * q) >> 3 : ((i + j) < (cw >> 1) ? (q >> 2) : (q >> 3));
        uint32_t a = ((uint32_t)abs(v) << sh) + rnd;
        uint32_t lv = (uint32_t)(((uint64_t)a * recip) >> 32);
        if (lv > 0x7FFF) lv = 0x7FFF;
        t->level[(i << bwl) + j] = v < 0 ? -(int32_t)lv : (int32_t)lv;
      }
  }
  for (c = 0; c < cw * cw; c++)
    if (t->level[scan[c]]) eob = c + 1;
  t->eob = eob;
  if (eob) {
    /* normative dequant §7.12.3 */
    int32_t *dq = coef;
    memset(dq, 0, sizeof(int32_t) * n * n);
    for (i = 0; i < cw; i++)
      for (j = 0; j < cw; j++) {
        int32_t lv = t->level[(i << bwl) + j];
        if (lv) {
          uint32_t q = qstep_at(e, plane, log2n, i, j, tx_type);
          int64_t d = ((int64_t)abs(lv) * q) & 0xFFFFFF;
          int64_t lim = (int64_t)1 << (7 + bd);
          d >>= sh;
          if (lv < 0) d = -d;
          if (d < -lim) d = -lim;
          if (d > lim - 1) d = lim - 1;
          dq[i * n + j] = (int32_t)d;
        }
      }
    av1o_inv_txfm2d_add(dq, rec, rstride, log2n, tx_type, bd, eob);
  }
  free(resid);
  return eob;
}

/* ------------------------------------------------------------------ inter prediction §7.11.3 */
typedef struct { int row, col; } Mv; /* 1/8 luma samples */

/* Block inter prediction (§7.11.3.4) for an unscaled single reference, frame-level interpolation filter:
 * BILINEAR (Subpel_Filters[3][p] = {0,0,0,128-8p,8p,0,0,0}) when cfg->subpel == 0, EIGHTTAP (Subpel_Filters[0], and
 * Subpel_Filters[4] - four taps - along a dimension of at most 4 samples) when cfg->subpel == 1.  Rounding InterRound0 = 3,
 * InterRound1 = 11 (8/10 bit, not compound).  Position of sample (i, j) in 1/16 plane samples: ((x0 + j) << 4) + mv_q4,
 * mv_q4 = (2*mv) >> subsampling (§7.11.3.3 with xScale = 1 << 14).  Reference samples are clamped to [0, last]. */
static void filter_taps(int eighttap, int n, int phase, int *f) {
  int t;
  if (eighttap) for (t = 0; t < 8; t++) f[t] = av1_subpel_filters[n <= 4][phase][t];
  else for (t = 0; t < 8; t++) f[t] = t == 3 ? 128 - 8 * phase : (t == 4 ? 8 * phase : 0);
}

static void interp_block(const Av1oFrame *ref, int plane, int last_x, int last_y, int x0, int y0, int n, Mv mv, int eighttap, int bd,
                         uint16_t *dst, int dstride) {
  const int ss = plane > 0;
  const int mvq_r = (2 * mv.row) >> ss, mvq_c = (2 * mv.col) >> ss;
  const int py = (y0 << 4) + mvq_r, px = (x0 << 4) + mvq_c;
  const int iy = py >> 4, fy = py & 15, ix = px >> 4, fx = px & 15;
  int32_t *mid = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 7) * n);
  int fh[8], fv[8];
  int r, c, t;
  filter_taps(eighttap, n, fx, fh);
  filter_taps(eighttap, n, fy, fv);
  for (r = 0; r < n + 7; r++)
    for (c = 0; c < n; c++) {
      int yy = iy + r - 3, sum = 0;
      yy = yy < 0 ? 0 : (yy > last_y ? last_y : yy);
      for (t = 0; t < 8; t++) {
        int xx = ix + c + t - 3;
        xx = xx < 0 ? 0 : (xx > last_x ? last_x : xx);
        sum += fh[t] * (int)ref->p[plane][(size_t)yy * ref->stride[plane] + xx];
      }
      mid[r * n + c] = (sum + 4) >> 3; /* Round2(sum, InterRound0) */
    }
  for (r = 0; r < n; r++)
    for (c = 0; c < n; c++) {
      int sum = 0, v;
      for (t = 0; t < 8; t++) sum += fv[t] * mid[(r + t) * n + c];
      v = (sum + 1024) >> 11; /* Round2(sum, InterRound1) */
      dst[r * dstride + c] = (uint16_t)(v < 0 ? 0 : (v > (1 << bd) - 1 ? (1 << bd) - 1 : v));
    }
  free(mid);
}

static void predict_inter(const Enc *e, int plane, int x0, int y0, int n, Mv mv, uint16_t *dst, int dstride) {
  const int ss = plane > 0;
  /* lastX / lastY of §7.11.3.3: the reference is clamped to the SIGNALLED frame size */
  interp_block(e->ref, plane, ((true_w(e->cfg) + ss) >> ss) - 1, ((true_h(e->cfg) + ss) >> ss) - 1, x0, y0, n, mv, e->cfg->subpel,
               e->cfg->bit_depth, dst, dstride);
}

/* Full search on luma, encoder-side, OPEN LOOP: the search compares the source block
 * with the previous SOURCE frame (e->prev_src), not with the reconstruction it will be predicted from - the vectors of
 * a whole chunk can then be searched up front, off the frame-by-frame reconstruction chain; its SAD
 * is also what the inter/intra decision uses.  Integer stage: cost = SAD(source, previous source displaced) +
 * n * (|dx| + |dy|); candidates keep the reference block within 16 samples of the frame (so no motion
 * vector ever needs the clamping of §7.10.2.14); ties go to the first candidate in (dy, dx) raster order.
 * cfg->subpel: two refinement stages around the winner, the 8 half-sample neighbours and then the 8 quarter-sample
 * neighbours of the stage's best, each interpolated from the previous source with the prediction's own filter
 * (EIGHTTAP, both roundings); cost = SATD (8x8 Hadamard, block_satd8) + (n * (|mv.row| + |mv.col|) >> 3) (the same
 * penalty in 1/8 units), the integer winner re-costed the same way; a candidate replaces the best only when strictly
 * cheaper, visited in (row, col) raster order; same 16-sample bound.
 * Returns the SAD of the chosen vector (what the inter/intra decision compares). */
static void hadamard8(int *v) {
  int t[8];
  t[0] = v[0] + v[4]; t[4] = v[0] - v[4]; t[1] = v[1] + v[5]; t[5] = v[1] - v[5]; t[2] = v[2] + v[6]; t[6] = v[2] - v[6]; t[3] = v[3] + v[7]; t[7] = v[3] - v[7];
  v[0] = t[0] + t[2]; v[2] = t[0] - t[2]; v[1] = t[1] + t[3]; v[3] = t[1] - t[3]; v[4] = t[4] + t[6]; v[6] = t[4] - t[6]; v[5] = t[5] + t[7]; v[7] = t[5] - t[7];
  t[0] = v[0] + v[1]; t[1] = v[0] - v[1]; t[2] = v[2] + v[3]; t[3] = v[2] - v[3]; t[4] = v[4] + v[5]; t[5] = v[4] - v[5]; t[6] = v[6] + v[7]; t[7] = v[6] - v[7];
  memcpy(v, t, sizeof(t));
}

/* SATD of the n x n block: sum of the absolute 8x8 Hadamard coefficients (H X H^T, H the +-1 matrix of order 8) of
 * (a - b) over all 8x8 sub-blocks, >> 3 (SURVEY.md §8a a13 "SATD (8x8 Hadamard) refinement"). */
static int block_satd8(const uint16_t *a, int as, const uint16_t *b, int bs, int n) {
  long total = 0;
  int by, bx, i, j;
  for (by = 0; by < n; by += 8)
    for (bx = 0; bx < n; bx += 8) {
      int m[8][8];
      for (i = 0; i < 8; i++) {
        for (j = 0; j < 8; j++) m[i][j] = (int)a[(by + i) * as + bx + j] - (int)b[(by + i) * bs + bx + j];
        hadamard8(m[i]);
      }
      for (j = 0; j < 8; j++) {
        int v[8];
        for (i = 0; i < 8; i++) v[i] = m[i][j];
        hadamard8(v);
        for (i = 0; i < 8; i++) total += abs(v[i]);
      }
    }
  return (int)(total >> 3);
}

/* Hierarchical motion search, first level (cfg->me_presearch; SURVEY.md §8a row a13 "hierarchical: 1/4-res ... full"): the
 * luma of the source and of the previous source at a quarter of the resolution - q(Y, X) = (sum of the 4x4 samples + 8) >> 4 - and per
 * 64x64 superblock a full search of its 16x16 quarter-resolution block over |dqx|, |dqy| <= 16 (+-64 luma samples): cost = SAD + 16 (|dqx|
 * + |dqy|), quarter-resolution coordinates clamped to the plane, ties to the first candidate in (dqy, dqx) raster order.  The winner,
 * rounded to whole multiples of 8 luma samples - C = ((dq + 1) >> 1) << 3 - is the CENTRE of the superblock's full-resolution search: every
 * leaf in it searches dx in [Cx - R, Cx + R], dy likewise, with the rules of the one-level search (cost with the absolute vector).  A
 * candidate is skipped when the superblock displaced by its centre would leave the frame by more than 16 samples (so the centre itself is
 * always a legal full-resolution candidate for every leaf). */
static void presearch_centres(Enc *e) {
  const int W = e->cfg->width, H = e->cfg->height, qw = W >> 2, qh = H >> 2;
  const int sb_cols = (W + 63) >> 6, sb_rows = (H + 63) >> 6;
  uint16_t *qc = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)qw * qh), *qp = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)qw * qh);
  int pass, y, x, i, j, sbr, sbc;
  for (pass = 0; pass < 2; pass++) {
    const Av1oFrame *f = pass ? e->prev_src : e->src;
    uint16_t *q = pass ? qp : qc;
    for (y = 0; y < qh; y++)
      for (x = 0; x < qw; x++) {
        int s = 8;
        for (i = 0; i < 4; i++)
          for (j = 0; j < 4; j++) s += f->p[0][(size_t)(4 * y + i) * f->stride[0] + 4 * x + j];
        q[(size_t)y * qw + x] = (uint16_t)(s >> 4);
      }
  }
  for (sbr = 0; sbr < sb_rows; sbr++)
    for (sbc = 0; sbc < sb_cols; sbc++) {
      const int sx = sbc * 64, sy = sbr * 64, sbw = W - sx < 64 ? W - sx : 64, sbh = H - sy < 64 ? H - sy : 64;
      long best_cost = -1;
      int bqx = 0, bqy = 0, dqy, dqx;
      for (dqy = -16; dqy <= 16; dqy++)
        for (dqx = -16; dqx <= 16; dqx++) {
          const int cx = ((dqx + 1) >> 1) * 8, cy = ((dqy + 1) >> 1) * 8;
          long sad = 0;
          if (sx + cx < -16 || sx + cx + sbw > W + 16 || sy + cy < -16 || sy + cy + sbh > H + 16) continue;
          for (i = 0; i < 16; i++)
            for (j = 0; j < 16; j++) {
              int ya = sy / 4 + i, xa = sx / 4 + j, yb = ya + dqy, xb = xa + dqx;
              ya = ya > qh - 1 ? qh - 1 : ya; xa = xa > qw - 1 ? qw - 1 : xa;
              yb = yb < 0 ? 0 : (yb > qh - 1 ? qh - 1 : yb); xb = xb < 0 ? 0 : (xb > qw - 1 ? qw - 1 : xb);
              sad += abs((int)qc[(size_t)ya * qw + xa] - (int)qp[(size_t)yb * qw + xb]);
            }
          sad += 16 * (abs(dqx) + abs(dqy));
          if (best_cost < 0 || sad < best_cost) { best_cost = sad; bqx = dqx; bqy = dqy; }
        }
      e->me_centre[2 * (sbr * sb_cols + sbc)] = (int16_t)(((bqy + 1) >> 1) * 8);
      e->me_centre[2 * (sbr * sb_cols + sbc) + 1] = (int16_t)(((bqx + 1) >> 1) * 8);
    }
  free(qc);
  free(qp);
}

static int motion_search(const Enc *e, int x, int y, int n, Mv *best) {
  const int R = e->cfg->me_range, W = e->cfg->width, H = e->cfg->height;
  /* centre of the search: zero, or the superblock's quarter-resolution winner (presearch_centres) */
  const int sbi = (y >> 6) * ((W + 63) >> 6) + (x >> 6);
  const int cdy = e->me_centre ? e->me_centre[2 * sbi] : 0, cdx = e->me_centre ? e->me_centre[2 * sbi + 1] : 0;
  const uint16_t *src = e->src->p[0] + (size_t)y * e->src->stride[0] + x;
  const uint16_t *ref = e->prev_src->p[0];
  const int rs = e->prev_src->stride[0], sstr = e->src->stride[0];
  long best_cost = -1;
  int best_sad = 0, dy, dx, i, j;
  best->row = best->col = 0;
  for (dy = cdy - R; dy <= cdy + R; dy++)
    for (dx = cdx - R; dx <= cdx + R; dx++) {
      int sad = 0;
      long cost;
      if (x + dx < -16 || x + dx + n > W + 16 || y + dy < -16 || y + dy + n > H + 16) continue;
      for (i = 0; i < n; i++) {
        int yy = y + dy + i;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        for (j = 0; j < n; j++) {
          int xx = x + dx + j;
          xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
          sad += abs((int)src[i * sstr + j] - (int)ref[(size_t)yy * rs + xx]);
        }
      }
      cost = (long)sad + (long)n * (abs(dx) + abs(dy));
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_sad = sad; best->row = dy * 8; best->col = dx * 8; }
    }
  if (e->cfg->subpel) {
    uint16_t *pred = (uint16_t *)malloc(sizeof(uint16_t) * n * n);
    int step;
    /* the refinement compares SATD: the integer winner's first */
    interp_block(e->prev_src, 0, W - 1, H - 1, x, y, n, *best, 1, e->cfg->bit_depth, pred, n);
    best_cost = (long)block_satd8(src, sstr, pred, n, n) + (((long)n * (abs(best->row) + abs(best->col))) >> 3);
    for (step = 4; step >= 2; step >>= 1) {
      const Mv base = *best;
      int dr, dc;
      for (dr = -step; dr <= step; dr += step)
        for (dc = -step; dc <= step; dc += step) {
          Mv mv;
          int sad = 0;
          long cost;
          if (!dr && !dc) continue;
          mv.row = base.row + dr; mv.col = base.col + dc;
          if (x * 8 + mv.col < -128 || (x + n) * 8 + mv.col > (W + 16) * 8 || y * 8 + mv.row < -128 || (y + n) * 8 + mv.row > (H + 16) * 8) continue;
          interp_block(e->prev_src, 0, W - 1, H - 1, x, y, n, mv, 1, e->cfg->bit_depth, pred, n);
          for (i = 0; i < n; i++)
            for (j = 0; j < n; j++) sad += abs((int)src[i * sstr + j] - (int)pred[i * n + j]);
          cost = (long)block_satd8(src, sstr, pred, n, n) + (((long)n * (abs(mv.row) + abs(mv.col))) >> 3);
          if (cost < best_cost) { best_cost = cost; best_sad = sad; *best = mv; }
        }
    }
    free(pred);
  }
  return best_sad;
}

/* ------------------------------------------------------------------ motion vector prediction §7.10.2 */
#define REF_CAT_LEVEL 640
#define MV_BORDER 128
typedef struct {
  Mv mv[10];
  int weight[10];
  int num;          /* NumMvFound */
  int new_count;    /* NewMvCount */
  int found_match;  /* FoundMatch */
  int new_ctx, ref_ctx, zero_ctx;
} MvStack;

static int is_inside(const Enc *e, int r, int c);

/* add_ref_mv_candidate + search_stack (§7.10.2.7/.8) for a single LAST_FRAME reference: a neighbour matches iff it
 * is inter (every inter block of this build references LAST_FRAME; RefFrame[1] = NONE) */
static void stack_add(const Enc *e, MvStack *s, int r, int c, int weight) {
  const size_t idx = (size_t)r * e->g->mi_cols + c;
  Mv m;
  int i;
  if (!e->mi_is_inter[idx]) return;
  m.row = e->mi_mv[2 * idx];
  m.col = e->mi_mv[2 * idx + 1];
  /* lower_mv_precision with allow_high_precision_mv = 0, force_integer_mv = 0 (§7.10.2.3) */
  if (m.row & 1) m.row += m.row > 0 ? -1 : 1;
  if (m.col & 1) m.col += m.col > 0 ? -1 : 1;
  if (e->mi_newmv[idx]) s->new_count++;
  s->found_match = 1;
  for (i = 0; i < s->num; i++)
    if (s->mv[i].row == m.row && s->mv[i].col == m.col) break;
  if (i < s->num) s->weight[i] += weight;
  else if (s->num < 8) { s->mv[s->num] = m; s->weight[s->num] = weight; s->num++; }
}
static int cand_n4(const Enc *e, int r, int c) { return (1 << e->mi_bsl[(size_t)r * e->g->mi_cols + c]) >> 2; }

static void scan_row(const Enc *e, MvStack *s, int mi_r, int mi_c, int bw4, int delta_row) {
  int delta_col = 0, i = 0;
  int end4 = bw4 < e->g->mi_cols - mi_c ? bw4 : e->g->mi_cols - mi_c;
  const int use16 = bw4 >= 16;
  if (end4 > 16) end4 = 16;
  if (abs(delta_row) > 1) { delta_row += mi_r & 1; delta_col = 1 - (mi_c & 1); }
  while (i < end4) {
    int r = mi_r + delta_row, c = mi_c + delta_col + i, len;
    if (!is_inside(e, r, c)) break;
    len = cand_n4(e, r, c);
    if (len > bw4) len = bw4;
    if (abs(delta_row) > 1 && len < 2) len = 2;
    if (use16 && len < 4) len = 4;
    stack_add(e, s, r, c, len * 2);
    i += len;
  }
}
static void scan_col(const Enc *e, MvStack *s, int mi_r, int mi_c, int bh4, int delta_col) {
  int delta_row = 0, i = 0;
  int end4 = bh4 < e->g->mi_rows - mi_r ? bh4 : e->g->mi_rows - mi_r;
  const int use16 = bh4 >= 16;
  if (end4 > 16) end4 = 16;
  if (abs(delta_col) > 1) { delta_row = 1 - (mi_r & 1); delta_col += mi_c & 1; }
  while (i < end4) {
    int r = mi_r + delta_row + i, c = mi_c + delta_col, len;
    if (!is_inside(e, r, c)) break;
    len = cand_n4(e, r, c);
    if (len > bh4) len = bh4;
    if (abs(delta_col) > 1 && len < 2) len = 2;
    if (use16 && len < 4) len = 4;
    stack_add(e, s, r, c, len * 2);
    i += len;
  }
}
/* scan_point (§7.10.2.4): the candidate must lie in the tile and have been decoded already */
static void scan_point(const Enc *e, MvStack *s, int mi_r, int mi_c, int dr, int dc) {
  int r = mi_r + dr, c = mi_c + dc;
  if (is_inside(e, r, c) && e->mi_bsl[(size_t)r * e->g->mi_cols + c] != 0) stack_add(e, s, r, c, 4);
}
static void sort_stack(MvStack *s, int start, int end) {
  while (end > start) {
    int new_end = start, i;
    for (i = start + 1; i < end; i++)
      if (s->weight[i - 1] < s->weight[i]) {
        Mv m = s->mv[i - 1]; int w = s->weight[i - 1];
        s->mv[i - 1] = s->mv[i]; s->weight[i - 1] = s->weight[i];
        s->mv[i] = m; s->weight[i] = w;
        new_end = i;
      }
    end = new_end;
  }
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* find_mv_stack (§7.10.2) for isCompound = 0, RefFrame = {LAST_FRAME, NONE}, identity global motion,
 * use_ref_frame_mvs = 0 */
static void build_mv_stack(const Enc *e, int mi_r, int mi_c, int bw4, int bh4, MvStack *s) {
  int found_above, found_left, close_matches, total_matches, num_nearest, num_new, i;
  memset(s, 0, sizeof(*s));
  scan_row(e, s, mi_r, mi_c, bw4, -1);
  found_above = s->found_match; s->found_match = 0;
  scan_col(e, s, mi_r, mi_c, bh4, -1);
  found_left = s->found_match; s->found_match = 0;
  if ((bw4 > bh4 ? bw4 : bh4) <= 16) scan_point(e, s, mi_r, mi_c, -1, bw4);
  if (s->found_match) found_above = 1;
  s->found_match = 0;
  close_matches = found_above + found_left;
  num_nearest = s->num;
  num_new = s->new_count;
  for (i = 0; i < num_nearest; i++) s->weight[i] += REF_CAT_LEVEL;
  s->zero_ctx = 0; /* no temporal candidates */
  scan_point(e, s, mi_r, mi_c, -1, -1);
  if (s->found_match) found_above = 1;
  s->found_match = 0;
  scan_row(e, s, mi_r, mi_c, bw4, -3);
  if (s->found_match) found_above = 1;
  s->found_match = 0;
  scan_col(e, s, mi_r, mi_c, bh4, -3);
  if (s->found_match) found_left = 1;
  s->found_match = 0;
  scan_row(e, s, mi_r, mi_c, bw4, -5);
  if (s->found_match) found_above = 1;
  s->found_match = 0;
  scan_col(e, s, mi_r, mi_c, bh4, -5);
  if (s->found_match) found_left = 1;
  s->found_match = 0;
  total_matches = found_above + found_left;
  sort_stack(s, 0, num_nearest);
  sort_stack(s, num_nearest, s->num);
  if (s->num < 2) {
    /* extra search (§7.10.2.12): neighbours with any reference; with a single reference in use it can only
     * meet vectors that are already in the list */
    int w4 = bw4 < e->g->mi_cols - mi_c ? bw4 : e->g->mi_cols - mi_c, h4 = bh4 < e->g->mi_rows - mi_r ? bh4 : e->g->mi_rows - mi_r;
    int num4 = w4 < h4 ? w4 : h4, pass;
    if (num4 > 16) num4 = 16;
    for (pass = 0; pass < 2; pass++) {
      int idx = 0;
      while (idx < num4 && s->num < 2) {
        int r = pass == 0 ? mi_r - 1 : mi_r + idx, c = pass == 0 ? mi_c + idx : mi_c - 1, k;
        size_t mi;
        if (!is_inside(e, r, c)) break;
        mi = (size_t)r * e->g->mi_cols + c;
        if (e->mi_is_inter[mi]) {
          Mv m;
          m.row = e->mi_mv[2 * mi]; m.col = e->mi_mv[2 * mi + 1];
          for (k = 0; k < s->num; k++)
            if (s->mv[k].row == m.row && s->mv[k].col == m.col) break;
          if (k == s->num) { s->mv[s->num] = m; s->weight[s->num] = 2; s->num++; }
        }
        idx += cand_n4(e, r, c);
      }
    }
    for (i = s->num; i < 2; i++) { s->mv[i].row = 0; s->mv[i].col = 0; } /* GlobalMvs[0] */
  }
  /* context_and_clamping (§7.10.2.14) */
  if (close_matches == 0) { s->new_ctx = total_matches < 1 ? total_matches : 1; s->ref_ctx = total_matches; }
  else if (close_matches == 1) { s->new_ctx = 3 - (num_new < 1 ? num_new : 1); s->ref_ctx = 2 + total_matches; }
  else { s->new_ctx = 5 - (num_new < 1 ? num_new : 1); s->ref_ctx = 5; }
  for (i = 0; i < s->num; i++) {
    int to_top = -(mi_r * 4) * 8, to_bottom = ((e->g->mi_rows - bh4 - mi_r) * 4) * 8;
    int to_left = -(mi_c * 4) * 8, to_right = ((e->g->mi_cols - bw4 - mi_c) * 4) * 8;
    s->mv[i].row = clampi(s->mv[i].row, to_top - (MV_BORDER + bh4 * 4 * 8), to_bottom + (MV_BORDER + bh4 * 4 * 8));
    s->mv[i].col = clampi(s->mv[i].col, to_left - (MV_BORDER + bw4 * 4 * 8), to_right + (MV_BORDER + bw4 * 4 * 8));
  }
}

static int drl_ctx(const MvStack *s, int idx) {
  if (s->weight[idx] >= REF_CAT_LEVEL && s->weight[idx + 1] >= REF_CAT_LEVEL) return 0;
  if (s->weight[idx] >= REF_CAT_LEVEL && s->weight[idx + 1] < REF_CAT_LEVEL) return 1;
  if (s->weight[idx] < REF_CAT_LEVEL && s->weight[idx + 1] < REF_CAT_LEVEL) return 2;
  return 0;
}

static void write_sym(struct Enc_ *e, int s, uint16_t *icdf, int n);
/* read_mv_component mirrored (§5.11.32): d = |component difference| in 1/8 samples, > 0 */
static void write_mv_component(struct Enc_ *e, int comp, int v) {
  TileCdfs *cdf = &e->cdf;
  const int sign = v < 0, mag = abs(v), z = mag - 1;
  int cls = 0, o, d, fr, hp;
  /* mv_class: class c > 0 covers offsets [16 << (c-1) ... ) in 1/8 units: base(c) = CLASS0_SIZE << (c + 2) */
  while (cls < 10 && z >= (2 << (cls + 3))) cls++;
  o = z - (cls ? (2 << (cls + 2)) : 0);
  d = o >> 3; fr = (o >> 1) & 3; hp = o & 1;
  write_sym(e, sign, cdf->mvc[comp].sign, 2);
  write_sym(e, cls, cdf->mvc[comp].cls, 11);
  if (cls == 0) {
    write_sym(e, d, cdf->mvc[comp].class0, 2);
    write_sym(e, fr, cdf->mvc[comp].class0_fp[d], 4);
  } else {
    int i;
    for (i = 0; i < cls; i++) write_sym(e, (d >> i) & 1, cdf->mvc[comp].bits[i], 2);
    write_sym(e, fr, cdf->mvc[comp].fp, 4);
  }
  (void)hp; /* allow_high_precision_mv = 0: hp = 1 is implied, every coded vector has odd offset */
}

/* ------------------------------------------------------------------ block coding §5.11.5 */
typedef struct { int ymode, yangle, uvmode, uvangle, cfl_au, cfl_av; } ModeDec;   /* cfl_a*: CflAlphaU / V, -16 .. 16 (uvmode == UV_CFL_PRED) */

static int block_sad(const uint16_t *a, int as, const uint16_t *b, int bs, int n) {
  int i, j, s = 0;
  for (i = 0; i < n; i++)
    for (j = 0; j < n; j++) s += abs((int)a[i * as + j] - (int)b[i * bs + j]);
  return s;
}

/* ---- chroma from luma (spec 7.11.5).  ac[i * nc + j] = subsampled reconstructed luma in Q3 minus its block average; the block's
 * own luma reconstruction is complete (one transform block per block, so MaxLumaW / MaxLumaH never clamp). */
static void cfl_luma_ac(const Enc *e, int x_l, int y_l, int log2nc, int16_t *ac) {
  const int nc = 1 << log2nc, st = e->rec->stride[0];
  const uint16_t *l = e->rec->p[0] + (size_t)y_l * st + x_l;
  int i, j, sum = 0, avg;
  for (i = 0; i < nc; i++)
    for (j = 0; j < nc; j++) {
      int t = l[(2 * i) * st + 2 * j] + l[(2 * i) * st + 2 * j + 1] + l[(2 * i + 1) * st + 2 * j] + l[(2 * i + 1) * st + 2 * j + 1];
      ac[i * nc + j] = (int16_t)(t << 1);
      sum += t << 1;
    }
  avg = (sum + (1 << (2 * log2nc - 1))) >> (2 * log2nc);
  for (i = 0; i < nc * nc; i++) ac[i] = (int16_t)(ac[i] - avg);
}
static int cfl_px(int dc, int alpha, int ac, int maxv) {
  const int s = alpha * ac, r = s >= 0 ? (s + 32) >> 6 : -((-s + 32) >> 6);   /* Round2Signed(alpha * ac, 6) */
  const int v = dc + r;
  return v < 0 ? 0 : (v > maxv ? maxv : v);
}
static int cfl_sad(const uint16_t *src, int sstride, const int16_t *ac, int nc, int dc, int alpha, int maxv) {
  int i, j, s = 0;
  for (i = 0; i < nc; i++)
    for (j = 0; j < nc; j++) s += abs((int)src[i * sstride + j] - cfl_px(dc, alpha, ac[i * nc + j], maxv));
  return s;
}
/* the encoder's alpha for one plane: least-squares estimate 8 * sum(a * d) / sum(a * a) with a = ac >> 3 and
 * d = source - dc, rounded to nearest and clamped to -16 .. 16; then the SAD of the estimate and its two neighbours, first minimum
 * in the order estimate, -1, +1 */
static int cfl_choose_alpha(const uint16_t *src, int sstride, const int16_t *ac, int nc, int dc, int maxv, int *sad_out) {
  long long num = 0, den = 0, t;
  int i, j, est, k, best = 0, best_sad = -1;
  for (i = 0; i < nc; i++)
    for (j = 0; j < nc; j++) {
      const int a = ac[i * nc + j] >> 3, d = (int)src[i * sstride + j] - dc;
      num += a * d; den += a * a;
    }
  if (den == 0) est = 0;
  else {
    t = 16 * num + den;   /* floor((16 num + den) / (2 den)) = round-half-up of 8 num / den */
    est = (int)(t >= 0 ? t / (2 * den) : -((-t + 2 * den - 1) / (2 * den)));
  }
  est = est < -16 ? -16 : (est > 16 ? 16 : est);
  for (k = 0; k < 3; k++) {
    int a = est + (k == 0 ? 0 : (k == 1 ? -1 : 1)), sad;
    a = a < -16 ? -16 : (a > 16 ? 16 : a);
    sad = cfl_sad(src, sstride, ac, nc, dc, a, maxv);
    if (best_sad < 0 || sad < best_sad) { best_sad = sad; best = a; }
  }
  *sad_out = best_sad;
  return best;
}

static void encode_block(Enc *e, int mi_r, int mi_c, int bsl /* log2 block size in px */) {
  const Av1oConfig *cfg = e->cfg;
  const Geom *g = e->g;
  const int n = 1 << bsl, bw4 = n >> 2;
  const int bd = cfg->bit_depth;
  const int avail_u = is_inside(e, mi_r - 1, mi_c), avail_l = is_inside(e, mi_r, mi_c - 1);
  const int sb_r = mi_r & 15, sb_c = mi_c & 15; /* within SB, luma 4x4 units */
  uint16_t edge_a[2 * 64 + 16], edge_l[2 * 64 + 16];
  uint16_t *pred = (uint16_t *)malloc(sizeof(uint16_t) * n * n);
  TxbCoefs *ty = (TxbCoefs *)malloc(sizeof(TxbCoefs) * 3);
  TxbCoefs *tu = ty + 1, *tv = ty + 2;
  ModeDec md = { DC_PRED, 0, DC_PRED, 0, 0, 0 };
  int plane, i, j, skip;
  int have_ar[2], have_bl[2];
  Av1oEdgeCtl ef[2];
  const int log2n_y = bsl, log2n_uv = bsl - 1 > 5 ? 5 : bsl - 1;
  int tx_y, tx_uv;
  /* inter frames: the block is either intra (as on key frames) or predicted from LAST_FRAME with `mv` */
  const int inter_frame = e->ref != NULL;
  int is_inter = 0, inter_mode = 0 /* 0 NEARESTMV 1 NEARMV 2 GLOBALMV 3 NEWMV */, sad_intra = 0, sad_inter = 0;
  Mv mv = { 0, 0 };
  MvStack stk;
  if (inter_frame) {
    build_mv_stack(e, mi_r, mi_c, bw4, bw4, &stk);
    sad_inter = motion_search(e, mi_c * 4, mi_r * 4, n, &mv);
  }

  /* haveAboveRt / haveBelowLft from BlockDecoded (§5.11.35), luma and chroma */
  for (plane = 0; plane < 2; plane++) {
    int ss = plane;
    int step = (plane ? (1 << log2n_uv) : n) >> 2;
    int r4 = sb_r >> ss, c4 = sb_c >> ss;
    have_ar[plane] = e->block_decoded[plane][r4 - 1 + 1][c4 + step + 1];
    have_bl[plane] = e->block_decoded[plane][r4 + step + 1][c4 - 1 + 1];
  }

  /* intra edge filter (spec 7.11.2.8 get_filter_type): is the block above / left predicted with a smooth mode?  (blocks are
   * at least 8x8, so the chroma neighbour is the block over / beside the same mi position) */
  for (plane = 0; plane < 2; plane++) {
    const uint8_t *modes = plane ? e->mi_uvmode : e->mi_ymode;
    int sm = 0;
    if (avail_u && !e->mi_is_inter[(mi_r - 1) * g->mi_cols + mi_c]) { int m = modes[(mi_r - 1) * g->mi_cols + mi_c]; sm |= m == SMOOTH_PRED || m == SMOOTH_V_PRED || m == SMOOTH_H_PRED; }
    if (avail_l && !e->mi_is_inter[mi_r * g->mi_cols + mi_c - 1]) { int m = modes[mi_r * g->mi_cols + mi_c - 1]; sm |= m == SMOOTH_PRED || m == SMOOTH_V_PRED || m == SMOOTH_H_PRED; }
    {
      const int np = plane ? 1 << log2n_uv : n, px = plane ? mi_c * 2 : mi_c * 4, py = plane ? mi_r * 2 : mi_r * 4;
      const int pw = plane ? cfg->width / 2 : cfg->width, ph = plane ? cfg->height / 2 : cfg->height;
      ef[plane].enable = cfg->intra_edge_filter; ef[plane].filter_type = sm;
      ef[plane].n_top = np < pw - px ? np : pw - px; ef[plane].n_left = np < ph - py ? np : ph - py;
    }
  }

  /* ---- luma mode decision: closed-loop prediction SAD */
  {
    int x = mi_c * 4, y = mi_r * 4, best = -1, m;
    const uint16_t *src = e->src->p[0] + (size_t)y * e->src->stride[0] + x;
    prepare_edges(e, 0, x, y, n, avail_l, avail_u, have_ar[0], have_bl[0], edge_a, edge_l);
    if (cfg->fuzz_modes) {
      md.ymode = (int)(fuzz_rand(e) % 13);
      while (!((cfg->mode_mask >> md.ymode) & 1)) md.ymode = (md.ymode + 1) % 13;
      md.yangle = (md.ymode >= V_PRED && md.ymode <= D67_PRED) ? (int)(fuzz_rand(e) % 7) - 3 : 0;
      md.uvmode = (int)(fuzz_rand(e) % 13);
      while (!((cfg->mode_mask >> md.uvmode) & 1)) md.uvmode = (md.uvmode + 1) % 13;
      md.uvangle = (md.uvmode >= V_PRED && md.uvmode <= D67_PRED) ? (int)(fuzz_rand(e) % 7) - 3 : 0;
    } else {
      /* closed-loop SAD over the candidate modes; DC is kept unless the best other
       * candidate at least halves its SAD (SAD alone over-rates directional modes on gradients). */
      int sad_dc = -1;
      for (m = 0; m < 13; m++) {
        int sad;
        if (!((cfg->mode_mask >> m) & 1)) continue;
        av1o_predict_intra_ef(pred, n, bsl, m, 0, edge_a, edge_l, avail_u, avail_l, bd, &ef[0]);
        sad = block_sad(src, e->src->stride[0], pred, n, n);
        if (m == DC_PRED) { sad_dc = sad; continue; }
        if (best < 0 || sad < best) { best = sad; md.ymode = m; }
      }
      if (sad_dc >= 0 && (best < 0 || 2 * (long)best >= (long)sad_dc)) { md.ymode = DC_PRED; best = sad_dc; }
      /* angle delta: a directional winner is refined over the deltas -1, +1, -2, +2, -3, +3 (3 degrees each);
       * a delta replaces the current one only when its SAD is strictly smaller */
      if (cfg->angle_delta && md.ymode >= V_PRED && md.ymode <= D67_PRED) {
        static const int order[6] = { -1, 1, -2, 2, -3, 3 };
        int k;
        for (k = 0; k < 6; k++) {
          int sad;
          av1o_predict_intra_ef(pred, n, bsl, md.ymode, order[k], edge_a, edge_l, avail_u, avail_l, bd, &ef[0]);
          sad = block_sad(src, e->src->stride[0], pred, n, n);
          if (sad < best) { best = sad; md.yangle = order[k]; }
        }
      }
      md.uvmode = md.ymode;
      md.uvangle = md.yangle;
      sad_intra = best;
    }
    /* ---- inter frames: motion-compensated prediction wins when its luma SAD is not larger */
    if (inter_frame) {
      if (cfg->fuzz_modes) {
        unsigned r = fuzz_rand(e);
        is_inter = (r & 3) != 0;
        switch ((r >> 2) & 3) {
          case 0: mv.row = mv.col = 0; break;
          case 1: if (stk.num >= 1) mv = stk.mv[0]; break;
          case 2: if (stk.num >= 2) mv = stk.mv[1]; break;
          default: {
            int R = cfg->me_range, dx = (int)(fuzz_rand(e) % (unsigned)(2 * R + 1)) - R, dy = (int)(fuzz_rand(e) % (unsigned)(2 * R + 1)) - R;
            mv.row = dy * 8; mv.col = dx * 8;
            if (cfg->subpel) { unsigned q = fuzz_rand(e); mv.row += 2 * (int)(q & 3); mv.col += 2 * (int)((q >> 2) & 3); }
          }
        }
      } else {
        is_inter = sad_inter <= sad_intra;
      }
    }
    if (is_inter) predict_inter(e, 0, x, y, n, mv, e->rec->p[0] + (size_t)y * e->rec->stride[0] + x, e->rec->stride[0]);
    else av1o_predict_intra_ef(e->rec->p[0] + (size_t)y * e->rec->stride[0] + x, e->rec->stride[0], bsl, md.ymode, md.yangle,
                               edge_a, edge_l, avail_u, avail_l, bd, &ef[0]);
  }
  tx_y = (log2n_y <= 4 && !is_inter) ? mode_to_txfm[md.ymode] : DCT_DCT;
  code_tx_block(e, 0, mi_c * 4, mi_r * 4, log2n_y, tx_y, ty, cfg->tx_search && !is_inter && log2n_y <= 4);
  /* ---- chroma from luma (cfg->cfl; blocks up to 32x32): decision-driven on key frames - CfL replaces the luma-derived chroma mode
   * when the sum of its two planes' prediction SADs (each plane at its chosen alpha) plus the chroma block width is smaller than
   * the regular mode's, and the alphas are not both zero (not codable); fuzzed streams take it at random on any frame */
  {
    const int nc = 1 << log2n_uv, x = mi_c * 2, y = mi_r * 2, maxv = (1 << bd) - 1;
    int16_t *ac = NULL;
    if (cfg->cfl && !is_inter && n <= 32) {
      if (cfg->fuzz_modes) {
        unsigned r = fuzz_rand(e);
        if (r % 3 == 0) {
          md.cfl_au = (int)((r >> 4) % 33) - 16; md.cfl_av = (int)((r >> 12) % 33) - 16;
          if (md.cfl_au == 0 && md.cfl_av == 0) md.cfl_av = 5;
          md.uvmode = UV_CFL_PRED; md.uvangle = 0;
        }
      } else if (!inter_frame) {
        int sad_cfl = 0, sad_reg = 0, au = 0, av = 0;
        ac = (int16_t *)malloc(sizeof(int16_t) * nc * nc);
        cfl_luma_ac(e, mi_c * 4, mi_r * 4, log2n_uv, ac);
        for (plane = 1; plane < 3; plane++) {
          const uint16_t *src = e->src->p[plane] + (size_t)y * e->src->stride[plane] + x;
          int sc, dc;
          prepare_edges(e, plane, x, y, nc, avail_l, avail_u, have_ar[1], have_bl[1], edge_a, edge_l);
          av1o_predict_intra_ef(pred, nc, log2n_uv, md.uvmode, md.uvangle, edge_a, edge_l, avail_u, avail_l, bd, &ef[1]);
          sad_reg += block_sad(src, e->src->stride[plane], pred, nc, nc);
          av1o_predict_intra(pred, nc, log2n_uv, DC_PRED, 0, edge_a, edge_l, avail_u, avail_l, bd);
          dc = pred[0];
          if (plane == 1) au = cfl_choose_alpha(src, e->src->stride[plane], ac, nc, dc, maxv, &sc);
          else av = cfl_choose_alpha(src, e->src->stride[plane], ac, nc, dc, maxv, &sc);
          sad_cfl += sc;
        }
        if ((au || av) && sad_cfl + nc < sad_reg) { md.uvmode = UV_CFL_PRED; md.uvangle = 0; md.cfl_au = au; md.cfl_av = av; }
      }
    }
    if (md.uvmode == UV_CFL_PRED && !ac) { ac = (int16_t *)malloc(sizeof(int16_t) * nc * nc); cfl_luma_ac(e, mi_c * 4, mi_r * 4, log2n_uv, ac); }
    tx_uv = (log2n_uv <= 4 && !is_inter) ? mode_to_txfm[md.uvmode] : DCT_DCT;
    for (plane = 1; plane < 3; plane++) {
      uint16_t *dst = e->rec->p[plane] + (size_t)y * e->rec->stride[plane] + x;
      if (is_inter) {
        predict_inter(e, plane, x, y, nc, mv, dst, e->rec->stride[plane]);
      } else {
        prepare_edges(e, plane, x, y, nc, avail_l, avail_u, have_ar[1], have_bl[1], edge_a, edge_l);
        if (md.uvmode == UV_CFL_PRED) {
          int dc;
          av1o_predict_intra(pred, nc, log2n_uv, DC_PRED, 0, edge_a, edge_l, avail_u, avail_l, bd);
          dc = pred[0];
          for (i = 0; i < nc; i++)
            for (j = 0; j < nc; j++) dst[i * e->rec->stride[plane] + j] = (uint16_t)cfl_px(dc, plane == 1 ? md.cfl_au : md.cfl_av, ac[i * nc + j], maxv);
        } else {
          av1o_predict_intra_ef(dst, e->rec->stride[plane], log2n_uv, md.uvmode, md.uvangle, edge_a, edge_l, avail_u, avail_l, bd, &ef[1]);
        }
      }
      code_tx_block(e, plane, x, y, log2n_uv, tx_uv, plane == 1 ? tu : tv, 0);
    }
    free(ac);
  }
  skip = ty->eob == 0 && tu->eob == 0 && tv->eob == 0;

  /* ---- syntax: intra_frame_mode_info */
  {
    int ctx = 0;
    if (avail_u) ctx += e->mi_skip[(mi_r - 1) * g->mi_cols + mi_c];
    if (avail_l) ctx += e->mi_skip[mi_r * g->mi_cols + mi_c - 1];
    WRITE_SYM(e, skip, e->cdf.skip[ctx], 2);
  }
  /* read_cdef: cdef_bits == 0 -> no literal, but remember that this SB has a coded cdef_idx */
  if (!skip && cfg->enable_cdef) e->cdef_idx_sb[(mi_r >> 4) * g->sb_cols + (mi_c >> 4)] = 0;
  if (inter_frame) {
    /* inter_frame_mode_info (§5.11.18): is_inter, context from the neighbours' intra-ness (§8.3.2) */
    const int a_intra = avail_u ? !e->mi_is_inter[(mi_r - 1) * g->mi_cols + mi_c] : 0;
    const int l_intra = avail_l ? !e->mi_is_inter[mi_r * g->mi_cols + mi_c - 1] : 0;
    int ctx;
    if (avail_u && avail_l) ctx = (l_intra && a_intra) ? 3 : ((l_intra || a_intra) ? 1 : 0);
    else if (avail_u || avail_l) ctx = 2 * (avail_u ? a_intra : l_intra);
    else ctx = 0;
    WRITE_SYM(e, is_inter, e->cdf.is_inter[ctx], 2);
  }
  if (is_inter) {
    /* inter_block_mode_info (§5.11.23): read_ref_frames -> LAST_FRAME = single_ref_p1 0, p3 0, p4 0.  Contexts
     * (§8.3.2) compare counts of reference names among the above/left blocks; only LAST_FRAME is ever used. */
    const int n_last = (avail_u ? e->mi_is_inter[(mi_r - 1) * g->mi_cols + mi_c] : 0) + (avail_l ? e->mi_is_inter[mi_r * g->mi_cols + mi_c - 1] : 0);
    const int rctx = n_last > 0 ? 2 : 1; /* ref_count_ctx(n_last, 0) */
    int pred_idx = 0;
    Mv pred;
    WRITE_SYM(e, 0, e->cdf.single_ref[0][rctx], 2); /* single_ref_p1: forward group */
    WRITE_SYM(e, 0, e->cdf.single_ref[2][rctx], 2); /* single_ref_p3: LAST/LAST2 */
    WRITE_SYM(e, 0, e->cdf.single_ref[3][rctx], 2); /* single_ref_p4: LAST */
    /* mode: the cheapest name of the chosen vector */
    if (stk.num >= 1 && mv.row == stk.mv[0].row && mv.col == stk.mv[0].col) inter_mode = 0;
    else if (stk.num >= 2 && mv.row == stk.mv[1].row && mv.col == stk.mv[1].col) inter_mode = 1;
    else if (mv.row == 0 && mv.col == 0) inter_mode = 2;
    else inter_mode = 3;
    WRITE_SYM(e, inter_mode != 3, e->cdf.newmv[stk.new_ctx], 2);                            /* new_mv: 0 = NEWMV */
    if (inter_mode != 3) {
      WRITE_SYM(e, inter_mode != 2, e->cdf.globalmv[stk.zero_ctx], 2);                      /* zero_mv: 0 = GLOBALMV */
      if (inter_mode != 2) WRITE_SYM(e, inter_mode == 1, e->cdf.refmv[stk.ref_ctx], 2);      /* ref_mv: 0 = NEARESTMV */
    }
    if (inter_mode == 3) {        /* NEWMV, RefMvIdx = 0 */
      if (stk.num > 1) WRITE_SYM(e, 0, e->cdf.drl[drl_ctx(&stk, 0)], 2);
    } else if (inter_mode == 1) { /* NEARMV, RefMvIdx = 1 */
      if (stk.num > 2) WRITE_SYM(e, 0, e->cdf.drl[drl_ctx(&stk, 1)], 2);
    }
    if (inter_mode == 3) {        /* read_mv: difference to RefStackMv[RefMvIdx] (GlobalMvs[0] = 0 when the list is empty) */
      int dr, dc, joint;
      pred = stk.mv[pred_idx];
      dr = mv.row - pred.row; dc = mv.col - pred.col;
      joint = (dr != 0 ? 2 : 0) | (dc != 0 ? 1 : 0); /* MV_JOINT_ZERO, HNZVZ, HZVNZ, HNZVNZ */
      WRITE_SYM(e, joint, e->cdf.mv_joint, 4);
      if (dr) write_mv_component(e, 0, dr);
      if (dc) write_mv_component(e, 1, dc);
    }
    /* interintra, motion mode, compound type, interpolation filter: nothing coded with this frame header */
  } else {
    if (inter_frame) {
      /* intra_block_mode_info (§5.11.22): y_mode by block-size group */
      WRITE_SYM(e, md.ymode, e->cdf.y_mode[bsl <= 3 ? 1 : (bsl == 4 ? 2 : 3)], 13);
    } else {
      int am = intra_mode_context[avail_u ? e->mi_ymode[(mi_r - 1) * g->mi_cols + mi_c] : DC_PRED];
      int lm = intra_mode_context[avail_l ? e->mi_ymode[mi_r * g->mi_cols + mi_c - 1] : DC_PRED];
      WRITE_SYM(e, md.ymode, e->cdf.kf_y_mode[am][lm], 13);
    }
    if (md.ymode >= V_PRED && md.ymode <= D67_PRED) WRITE_SYM(e, md.yangle + 3, e->cdf.angle_delta[md.ymode - V_PRED], 7);
    {
      int cfl_allowed = n <= 32;
      WRITE_SYM(e, md.uvmode, e->cdf.uv_mode[cfl_allowed][md.ymode], cfl_allowed ? 14 : 13);
    }
    if (md.uvmode >= V_PRED && md.uvmode <= D67_PRED) WRITE_SYM(e, md.uvangle + 3, e->cdf.angle_delta[md.uvmode - V_PRED], 7);
    if (md.uvmode == UV_CFL_PRED) {   /* read_cfl_alphas, spec 5.11.45: joint sign (zero / negative / positive per plane), then |alpha| - 1 */
      const int su = md.cfl_au == 0 ? 0 : (md.cfl_au < 0 ? 1 : 2), sv = md.cfl_av == 0 ? 0 : (md.cfl_av < 0 ? 1 : 2);
      WRITE_SYM(e, su * 3 + sv - 1, e->cdf.cfl_sign, 8);
      if (su) WRITE_SYM(e, abs(md.cfl_au) - 1, e->cdf.cfl_alpha[(su - 1) * 3 + sv], 16);
      if (sv) WRITE_SYM(e, abs(md.cfl_av) - 1, e->cdf.cfl_alpha[(sv - 1) * 3 + su], 16);
    }
  }
  /* (palette: allow_screen_content_tools = 0; filter intra: disabled; tx_size: TX_MODE_LARGEST) */

  /* ---- residual */
  if (skip) {
    /* reset_block_context */
    for (plane = 0; plane < 3; plane++) {
      int ss = plane > 0, w4 = bw4 >> ss ? bw4 >> ss : 1;
      int x4 = mi_c >> ss, y4 = (mi_r & 15) >> ss;
      for (i = 0; i < w4; i++) {
        e->above_lvl[plane][x4 + i] = 0; e->above_dc[plane][x4 + i] = 0;
        e->left_lvl[plane][y4 + i] = 0;  e->left_dc[plane][y4 + i] = 0;
      }
    }
  } else {
    write_coeffs(e, 0, log2n_y, mi_c, sb_r, mi_r, ty, md.ymode, 1, is_inter);
    write_coeffs(e, 1, log2n_uv, mi_c >> 1, sb_r >> 1, mi_r >> 1, tu, md.ymode, 1, is_inter);
    write_coeffs(e, 2, log2n_uv, mi_c >> 1, sb_r >> 1, mi_r >> 1, tv, md.ymode, 1, is_inter);
  }
  /* ---- bookkeeping */
  for (i = 0; i < bw4; i++)
    for (j = 0; j < bw4; j++) {
      int idx = (mi_r + i) * g->mi_cols + mi_c + j;
      if (mi_r + i < g->mi_rows && mi_c + j < g->mi_cols) {
        e->mi_bsl[idx] = (uint8_t)bsl;
        e->mi_skip[idx] = (uint8_t)skip;
        e->mi_ymode[idx] = (uint8_t)md.ymode;
        e->mi_uvmode[idx] = (uint8_t)md.uvmode;
        e->mi_is_inter[idx] = (uint8_t)is_inter;
        e->mi_newmv[idx] = (uint8_t)(is_inter && inter_mode == 3);
        e->mi_mv[2 * idx] = (int16_t)(is_inter ? mv.row : 0);
        e->mi_mv[2 * idx + 1] = (int16_t)(is_inter ? mv.col : 0);
      }
    }
  for (plane = 0; plane < 2; plane++) {
    int ss = plane, w4 = (bw4 >> ss) ? (bw4 >> ss) : 1;
    int r4 = sb_r >> ss, c4 = sb_c >> ss, pl2;
    for (pl2 = plane; pl2 < (plane ? 3 : 1); pl2++)
      for (i = 0; i < w4; i++)
        for (j = 0; j < w4; j++) e->block_decoded[pl2][r4 + i + 1][c4 + j + 1] = 1;
  }
  if (e->stats) {
    e->stats->n_blocks++;
    e->stats->n_skip_blocks += (uint64_t)skip;
    if (is_inter) { e->stats->n_inter_blocks++; e->stats->inter_mode_hist[inter_mode]++; }
    else e->stats->mode_hist[md.ymode]++;
    e->stats->bs_hist[bsl]++;
  }
  free(pred);
  free(ty);
}

/* ------------------------------------------------------------------ loop restoration syntax §5.11.57/58 */
static void write_lit_bits(Enc *e, unsigned v, int n) { if (n > 0) av1o_ec_encode_literal(&e->ec, v, n); }
/* NS(n) with literal bools (§4.10.10 mirrored) */
static void write_ns_bools(Enc *e, int n, int v) {
  int w = 0, x = n, m;
  while (x) { w++; x >>= 1; }
  m = (1 << w) - n;
  if (v < m) write_lit_bits(e, (unsigned)v, w - 1);
  else { int extra = v + m; write_lit_bits(e, (unsigned)(extra >> 1), w - 1); write_lit_bits(e, (unsigned)(extra & 1), 1); }
}
/* decode_subexp_bool mirrored: numSyms, k, value v in [0, numSyms) */
static void write_subexp_bools(Enc *e, int num_syms, int k, int v) {
  int i = 0, mk = 0;
  for (;;) {
    int b2 = i ? k + i - 1 : k, a = 1 << b2;
    if (num_syms <= mk + 3 * a) { write_ns_bools(e, num_syms - mk, v - mk); return; }
    if (v >= mk + a) { write_lit_bits(e, 1, 1); i++; mk += a; }   /* subexp_more_bools = 1 */
    else { write_lit_bits(e, 0, 1); write_lit_bits(e, (unsigned)(v - mk), b2); return; }
  }
}
static int recenter(int r, int v) { /* inverse of inverse_recenter */
  if (v > 2 * r) return v;
  if (v >= r) return (v - r) << 1;
  return ((r - v) << 1) - 1;
}
/* decode_signed_subexp_with_ref_bool mirrored: value v in [low, high), reference r */
static void write_signed_subexp_ref(Enc *e, int low, int high, int k, int r, int v) {
  const int mx = high - low;
  int x = v - low, rr = r - low;
  if ((rr << 1) <= mx) write_subexp_bools(e, mx, k, recenter(rr, x));
  else write_subexp_bools(e, mx, k, recenter(mx - 1 - rr, mx - 1 - x));
}
/* read_lr (§5.11.57) for the 64x64 superblock at (mi_r, mi_c): luma units whose origin lies in it */
static void write_lr(Enc *e, int mi_r, int mi_c) {
  static const int tmin[3] = { -5, -23, -17 }, tmax[3] = { 10, 8, 46 }, tk[3] = { 1, 2, 3 };
  const int urows = av1o_lr_units(true_h(e->cfg)), ucols = av1o_lr_units(true_w(e->cfg));
  int r0 = (mi_r * 4 + 63) / 64, r1 = ((mi_r + 16) * 4 + 63) / 64, c0 = (mi_c * 4 + 63) / 64, c1 = ((mi_c + 16) * 4 + 63) / 64, ur, uc, pass, j;
  if (!e->cfg->enable_lr || !e->lr_units) return;
  if (r1 > urows) r1 = urows;
  if (c1 > ucols) c1 = ucols;
  for (ur = r0; ur < r1; ur++)
    for (uc = c0; uc < c1; uc++) {
      const Av1oLrUnit *u = &e->lr_units[ur * ucols + uc];
      if (e->cfg->enable_lr == 2) WRITE_SYM(e, u->type, e->cdf.restoration_type, 3); /* restoration_type: NONE, WIENER, SGRPROJ */
      else WRITE_SYM(e, u->type, e->cdf.use_wiener, 2);
      if (!u->type) continue;
      if (u->type == 2) { /* §5.11.58 read_lr_unit, RESTORE_SGRPROJ */
        static const int xmin[2] = { -96, -32 }, xmax[2] = { 31, 95 };
        int i;
        write_lit_bits(e, (unsigned)u->sgr_set, 4); /* lr_sgr_set */
        for (i = 0; i < 2; i++) {
          if (av1o_sgr_params[u->sgr_set][i * 2]) write_signed_subexp_ref(e, xmin[i], xmax[i] + 1, 4, e->ref_sgr[i], u->sgr_xqd[i]);
          /* radius 0: not coded; the decoder derives 0 (pass 0) or Clip3(min, max, 128 - RefSgrXqd[0]) (pass 1) */
          e->ref_sgr[i] = u->sgr_xqd[i];
        }
        continue;
      }
      for (pass = 0; pass < 2; pass++)
        for (j = 0; j < 3; j++) {
          write_signed_subexp_ref(e, tmin[j], tmax[j] + 1, tk[j], e->ref_lr[pass][j], u->coef[pass][j]);
          e->ref_lr[pass][j] = u->coef[pass][j];
        }
    }
}

/* ------------------------------------------------------------------ partition §5.11.4 */
static int icdf_prob(const uint16_t *icdf, int el) { return (el > 0 ? icdf[el - 1] : 32768) - icdf[el]; }

/* Content-driven split decision (cfg->partition_search; SURVEY.md §8a row a10 "19 block sizes" - the decision SVT-AV1
 * spends most of `--preset 3` on, av1an.rs:14).  Open loop, from the SOURCE luma alone (so that the HIP path takes it for all frames of a
 * chunk in one pass before the tile walks): the node of size n at (x, y) splits when its four quadrants differ in ACTIVITY - the largest
 * quadrant variance exceeds four times the smallest plus (ac_q / 16)^2, about half a quantiser step in the sample domain, squared: an edge
 * or a textured object in one corner of an otherwise quiet block.  (A difference in LEVEL between the quadrants is no reason to split:
 * gradients predict and transform well in large blocks - measured on the 1080p clip, splitting on it coded 60 % more bytes.)
 * Sums over the quadrants' samples as the decoder will see the block: coordinates beyond the frame repeat its last column / row.
 * Integer only: S = sum, Q = sum of squares, V = m Q - S^2 = m^2 x variance (m = samples per quadrant). */
static int partition_wants_split(const Enc *e, int x, int y, int n) {
  const int h = n >> 1, w_ = e->cfg->width, h_ = e->cfg->height, st = e->src->stride[0];
  const uint16_t *p = e->src->p[0];
  const int64_t m = (int64_t)h * h, t = e->ac_q >> 4;
  int64_t vmin = INT64_MAX, vmax = 0;
  int q, i, j;
  for (q = 0; q < 4; q++) {
    const int x0 = x + (q & 1) * h, y0 = y + (q >> 1) * h;
    int64_t S = 0, Q = 0, V;
    for (i = 0; i < h; i++) {
      const int yy = y0 + i < h_ ? y0 + i : h_ - 1;
      for (j = 0; j < h; j++) {
        const int xx = x0 + j < w_ ? x0 + j : w_ - 1;
        const int64_t v = p[(size_t)yy * st + xx];
        S += v; Q += v * v;
      }
    }
    V = m * Q - S * S;
    if (V < vmin) vmin = V;
    if (V > vmax) vmax = V;
  }
  return vmax > 4 * vmin + t * t * m * m;
}

static void encode_partition(Enc *e, int mi_r, int mi_c, int bsl) {
  const Geom *g = e->g;
  const Av1oConfig *cfg = e->cfg;
  int n4 = 1 << (bsl - 2), half = n4 >> 1;
  int has_rows, has_cols, split, ctx, bsl_idx;
  uint16_t *pc;
  if (mi_r >= g->mi_rows || mi_c >= g->mi_cols) return;
  has_rows = (mi_r + half) < g->mi_rows;
  has_cols = (mi_c + half) < g->mi_cols;
  /* encoder decision: a node is a leaf iff its size is <= max_bs and the syntax lets it be one, i.e. its
   * half point lies inside the frame both ways (has_rows && has_cols).  Such a block may OVERHANG the frame edge by less
   * than half its size (1080 = 16 x 64 + 56: the bottom 32x32 blocks cover rows 1056..1087); the decoder reconstructs the
   * whole block and keeps what is inside, the encoder sees the source extended by replication there. */
  if (bsl <= cfg->min_bs_log2 || bsl == 3) split = 0;
  else if (bsl > cfg->max_bs_log2) split = 1;
  else split = cfg->partition_search ? partition_wants_split(e, mi_c * 4, mi_r * 4, 1 << bsl) : 0;
  if (!has_rows || !has_cols) split = 1;
  if (bsl == 3) split = 0;
  /* context (§8.3.2 partition): neighbours' block sizes */
  {
    int avail_u = is_inside(e, mi_r - 1, mi_c), avail_l = is_inside(e, mi_r, mi_c - 1);
    int above = avail_u && e->mi_bsl[(mi_r - 1) * g->mi_cols + mi_c] < bsl;
    int left = avail_l && e->mi_bsl[mi_r * g->mi_cols + mi_c - 1] < bsl;
    ctx = left * 2 + above;
  }
  bsl_idx = bsl - 3; /* 8x8 -> 0 ... 64x64 -> 3 */
  pc = e->cdf.partition[bsl_idx * 4 + ctx];
  if (has_rows && has_cols) {
    WRITE_SYM(e, split ? PARTITION_SPLIT : PARTITION_NONE, pc, bsl == 3 ? 4 : 10);
  } else if (has_cols) {
    /* split_or_horz: P(split) gathered from the vert-alike partitions (no adaptation) */
    int p = icdf_prob(pc, 2) + icdf_prob(pc, 3);
    if (bsl != 3) p += icdf_prob(pc, 4) + icdf_prob(pc, 6) + icdf_prob(pc, 7) + icdf_prob(pc, 9);
    av1o_ec_encode_bool(&e->ec, 1, (unsigned)p); /* must split (block crosses the bottom edge) */
    split = 1;
  } else if (has_rows) {
    int p = icdf_prob(pc, 1) + icdf_prob(pc, 3);
    if (bsl != 3) p += icdf_prob(pc, 4) + icdf_prob(pc, 5) + icdf_prob(pc, 6) + icdf_prob(pc, 8);
    av1o_ec_encode_bool(&e->ec, 1, (unsigned)p);
    split = 1;
  } else {
    split = 1;
  }
  if (!split) {
    encode_block(e, mi_r, mi_c, bsl);
  } else {
    encode_partition(e, mi_r, mi_c, bsl - 1);
    encode_partition(e, mi_r, mi_c + half, bsl - 1);
    encode_partition(e, mi_r + half, mi_c, bsl - 1);
    encode_partition(e, mi_r + half, mi_c + half, bsl - 1);
  }
}

static void clear_block_decoded(Enc *e, int mi_r, int mi_c) {
  int plane, y, x;
  for (plane = 0; plane < 3; plane++) {
    int ss = plane > 0;
    int sbw4 = (e->mi_col_end - mi_c) >> ss, sbh4 = (e->mi_row_end - mi_r) >> ss, sz = 16 >> ss;
    for (y = -1; y <= sz; y++)
      for (x = -1; x <= sz; x++) {
        int v;
        if (y < 0 && x < sbw4) v = 1;
        else if (x < 0 && y < sbh4) v = 1;
        else v = 0;
        e->block_decoded[plane][y + 1][x + 1] = (uint8_t)v;
      }
    e->block_decoded[plane][sz + 1][0] = 0;
  }
}

static size_t encode_tile(Enc *e, int tr, int tc, uint8_t *out, size_t cap) {
  const Geom *g = e->g;
  int r, c, p;
  e->mi_row_start = g->row_start_sb[tr] * 16;
  e->mi_row_end = g->row_start_sb[tr + 1] * 16 < g->mi_rows ? g->row_start_sb[tr + 1] * 16 : g->mi_rows;
  e->mi_col_start = g->col_start_sb[tc] * 16;
  e->mi_col_end = g->col_start_sb[tc + 1] * 16 < g->mi_cols ? g->col_start_sb[tc + 1] * 16 : g->mi_cols;
  init_cdfs(&e->cdf, e->cfg->base_q_idx);
  for (p = 0; p < 2; p++) { e->ref_lr[p][0] = 3; e->ref_lr[p][1] = -7; e->ref_lr[p][2] = 15; } /* Wiener_Taps_Mid */
  e->ref_sgr[0] = -32; e->ref_sgr[1] = 31; /* Sgrproj_Xqd_Mid */
  av1o_ec_init(&e->ec, out, cap);
  for (p = 0; p < 3; p++) {
    memset(e->above_lvl[p], 0, (size_t)g->mi_cols + 16);
    memset(e->above_dc[p], 0, (size_t)g->mi_cols + 16);
  }
  for (r = e->mi_row_start; r < e->mi_row_end; r += 16) {
    memset(e->left_lvl, 0, sizeof(e->left_lvl));
    memset(e->left_dc, 0, sizeof(e->left_dc));
    for (c = e->mi_col_start; c < e->mi_col_end; c += 16) {
      clear_block_decoded(e, r, c);
      write_lr(e, r, c);
      encode_partition(e, r, c, 6);
    }
  }
  {
    size_t n = av1o_ec_finish(&e->ec);
    if (e->stats) e->stats->n_symbols += e->ec.nsym;
    return e->ec.error ? (size_t)-1 : n;
  }
}

/* ------------------------------------------------------------------ frame */
long av1o_encode_frame(const Av1oConfig *cfg, const Av1oFrame *src, int with_seq_hdr, uint8_t *out, size_t out_cap,
                       Av1oFrame *recon, Av1oStats *stats) {
  return av1o_encode_frame2(cfg, src, NULL, NULL, with_seq_hdr, out, out_cap, recon, stats);
}

/* a frame of logical size w x h whose planes are allocated up to the next multiple of 64 both ways: blocks that overhang the
 * frame edge (encode_partition) read the replicated source and write their reconstruction there */
static Av1oFrame *frame_alloc_overhang(int w, int h) {
  Av1oFrame *f = (Av1oFrame *)calloc(1, sizeof(*f));
  const int aw = (w + 63) & ~63, ah = (h + 63) & ~63;
  int p;
  f->w = w;
  f->h = h;
  for (p = 0; p < 3; p++) {
    f->stride[p] = p ? aw / 2 : aw;
    f->p[p] = (uint16_t *)calloc((size_t)f->stride[p] * (p ? ah / 2 : ah), sizeof(uint16_t));
  }
  return f;
}
/* `in` (w x h) copied into such a frame, its last column / row replicated over the allocated margin */
static Av1oFrame *frame_extend_overhang(const Av1oFrame *in, int w, int h) {
  Av1oFrame *o = frame_alloc_overhang(w, h);
  const int aw = (w + 63) & ~63, ah = (h + 63) & ~63;
  int p, x, y;
  for (p = 0; p < 3; p++) {
    int ss = p > 0, pw = w >> ss, ph = h >> ss, paw = aw >> ss, pah = ah >> ss;
    for (y = 0; y < pah; y++)
      for (x = 0; x < paw; x++)
        o->p[p][(size_t)y * o->stride[p] + x] = in->p[p][(size_t)(y < ph ? y : ph - 1) * in->stride[p] + (x < pw ? x : pw - 1)];
  }
  return o;
}

/* copy `in` (iw x ih luma) into a new frame of ow x oh, replicating the last column / row */
static Av1oFrame *pad_frame(const Av1oFrame *in, int iw, int ih, int ow, int oh) {
  Av1oFrame *o = av1o_frame_alloc(ow, oh);
  int p, x, y;
  for (p = 0; p < 3; p++) {
    int ss = p > 0, piw = iw >> ss, pih = ih >> ss, pow_ = ow >> ss, poh = oh >> ss;
    for (y = 0; y < poh; y++)
      for (x = 0; x < pow_; x++)
        o->p[p][(size_t)y * o->stride[p] + x] = in->p[p][(size_t)(y < pih ? y : pih - 1) * in->stride[p] + (x < piw ? x : piw - 1)];
  }
  return o;
}

long av1o_encode_frame2(const Av1oConfig *cfg, const Av1oFrame *src, const Av1oFrame *ref, const Av1oFrame *prev_src, int with_seq_hdr,
                        uint8_t *out, size_t out_cap, Av1oFrame *recon, Av1oStats *stats) {
  if (!cfg->true_width && ((cfg->width & 7) || (cfg->height & 7))) {
    /* not a multiple of 8: run at the padded size, signal the true one; frames at this interface keep the true size */
    const int w = cfg->width, h = cfg->height, cw = (w + 7) & ~7, ch = (h + 7) & ~7;
    Av1oConfig c2 = *cfg;
    Av1oFrame *s2, *r2 = NULL, *p2 = NULL, *o2 = NULL;
    long n;
    int p, y;
    if ((w & 1) || (h & 1) || w < 8 || h < 8) return -2;
    c2.width = cw; c2.height = ch; c2.true_width = w; c2.true_height = h;
    s2 = pad_frame(src, w, h, cw, ch);
    if (ref) r2 = pad_frame(ref, w, h, cw, ch);
    if (prev_src) p2 = pad_frame(prev_src, w, h, cw, ch);
    if (recon) o2 = av1o_frame_alloc(cw, ch);
    n = av1o_encode_frame2(&c2, s2, r2, p2, with_seq_hdr, out, out_cap, o2, stats);
    if (recon && n >= 0)
      for (p = 0; p < 3; p++)
        for (y = 0; y < (h >> (p > 0)); y++)
          memcpy(recon->p[p] + (size_t)y * recon->stride[p], o2->p[p] + (size_t)y * o2->stride[p], sizeof(uint16_t) * (size_t)(w >> (p > 0)));
    av1o_frame_free(s2); av1o_frame_free(r2); av1o_frame_free(p2); av1o_frame_free(o2);
    return n;
  }
  Geom g;
  Enc *e;
  Av1oFrame *src_ext = NULL;
  Av1oLrUnit *lr_units = NULL;
  Av1oFrame *lr_out = NULL;
  size_t pos = 0, payload_cap, hdr_bits, n_mi;
  uint8_t *payload, *tilebuf;
  int tr, tc, p, bd = cfg->bit_depth;
  long ret = -1;
  if (cfg->width % 8 || cfg->height % 8 || cfg->width < 8 || cfg->height < 8) return -2;
  if (bd != 8 && bd != 10) return -2;
  /* base_q_idx 0 (no delta-q, no segmentation) makes the frame CodedLossless (spec 5.9.2): a different header and 4x4 WHT blocks,
   * which this reference does not write - refused like the product's cq_level 0 */
  if (cfg->base_q_idx < 1 || cfg->base_q_idx > 255) return -2;
  if (cfg->still_picture && ref) return -2;
  if (ref && !prev_src) return -2;
  make_geom(cfg, &g);
  if (g.tile_cols > 64 || g.tile_rows > 64) return -3;
  e = (Enc *)calloc(1, sizeof(Enc));
  e->cfg = cfg;
  e->g = &g;
  src_ext = frame_extend_overhang(src, cfg->width, cfg->height);
  e->src = src_ext;
  e->rec = frame_alloc_overhang(cfg->width, cfg->height);
  n_mi = (size_t)g.mi_rows * g.mi_cols;
  e->mi_bsl = (uint8_t *)calloc(n_mi, 1);
  e->mi_skip = (uint8_t *)calloc(n_mi, 1);
  e->mi_ymode = (uint8_t *)calloc(n_mi, 1);
  e->mi_uvmode = (uint8_t *)calloc(n_mi, 1);
  e->ref = ref;
  e->prev_src = prev_src;
  e->me_centre = NULL;
  e->mi_is_inter = (uint8_t *)calloc(n_mi, 1);
  e->mi_newmv = (uint8_t *)calloc(n_mi, 1);
  e->mi_mv = (int16_t *)calloc(n_mi * 2, sizeof(int16_t));
  e->cdef_idx_sb = (int8_t *)malloc((size_t)g.sb_rows * g.sb_cols);
  memset(e->cdef_idx_sb, -1, (size_t)g.sb_rows * g.sb_cols);
  for (p = 0; p < 3; p++) {
    e->above_lvl[p] = (uint8_t *)calloc((size_t)g.mi_cols + 16, 1);
    e->above_dc[p] = (uint8_t *)calloc((size_t)g.mi_cols + 16, 1);
  }
  e->dc_q = bd == 8 ? av1_dc_q8[cfg->base_q_idx] : av1_dc_q10[cfg->base_q_idx];
  e->ac_q = bd == 8 ? av1_ac_q8[cfg->base_q_idx] : av1_ac_q10[cfg->base_q_idx];
  e->stats = stats;
  e->rng_state = (uint32_t)(cfg->fuzz_coeffs ? cfg->fuzz_coeffs : (cfg->fuzz_modes ? cfg->fuzz_modes : 1)) * 2654435761u + 1u;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (cfg->me_presearch && ref && prev_src) {
    e->me_centre = (int16_t *)calloc((size_t)g.sb_rows * g.sb_cols * 2, sizeof(int16_t));
    presearch_centres(e);
  }

  payload_cap = (size_t)cfg->width * cfg->height * 4 + (size_t)g.tile_cols * g.tile_rows * 64 + 4096;
  payload = (uint8_t *)malloc(payload_cap);
  tilebuf = (uint8_t *)malloc(payload_cap);

  /* temporal delimiter + optional sequence header */
  if (out_cap < 64) goto done;
  out[pos++] = (2 << 3) | 2;
  out[pos++] = 0;
  if (with_seq_hdr) {
    long k = av1o_write_sequence_header(cfg, out + pos, out_cap - pos);
    if (k < 0) goto done;
    pos += (size_t)k;
  }
  /* Loop restoration: the unit decisions are coded at the head of each superblock but depend on the CDEF output of
   * the whole frame, so the tiles are run once to reconstruct (bits discarded), the units decided, then run again. */
  if (cfg->enable_lr) {
    Av1oFrame *cd = av1o_frame_alloc(cfg->width, cfg->height);
    for (tr = 0; tr < g.tile_rows; tr++)
      for (tc = 0; tc < g.tile_cols; tc++)
        if (encode_tile(e, tr, tc, tilebuf, payload_cap) == (size_t)-1) { av1o_frame_free(cd); goto done; }
    { int lv[4]; av1o_deblock_levels(cfg, ref == NULL, lv); av1o_deblock_frame(cfg, e->rec, e->mi_bsl, e->mi_skip, e->mi_is_inter, g.mi_cols, lv, cfg->deblock == 2 ? cfg->lf_sharpness : 0); }
    av1o_cdef_frame(cfg, e->rec, cd, e->mi_skip, g.mi_cols, e->cdef_idx_sb);
    lr_units = (Av1oLrUnit *)calloc((size_t)av1o_lr_units(true_w(cfg)) * av1o_lr_units(true_h(cfg)), sizeof(Av1oLrUnit));
    lr_out = av1o_frame_alloc(cfg->width, cfg->height);
    av1o_lr_frame(cfg, e->rec, cd, src, lr_out, lr_units, cfg->fuzz_modes ? (unsigned)cfg->fuzz_modes + 77u : 0u);
    av1o_frame_free(cd);
    e->lr_units = lr_units;
    memset(e->mi_bsl, 0, n_mi); memset(e->mi_skip, 0, n_mi); memset(e->mi_ymode, 0, n_mi); memset(e->mi_uvmode, 0, n_mi);
    memset(e->mi_is_inter, 0, n_mi); memset(e->mi_newmv, 0, n_mi); memset(e->mi_mv, 0, n_mi * 2 * sizeof(int16_t));
    memset(e->cdef_idx_sb, -1, (size_t)g.sb_rows * g.sb_cols);
    e->rng_state = (uint32_t)(cfg->fuzz_coeffs ? cfg->fuzz_coeffs : (cfg->fuzz_modes ? cfg->fuzz_modes : 1)) * 2654435761u + 1u;
    if (stats) memset(stats, 0, sizeof(*stats));
  }
  /* OBU_FRAME payload = frame_header_obu + byte_alignment + tile_group_obu */
  {
    size_t pp;
    BitW b;
    hdr_bits = frame_header_bits(cfg, &g, ref != NULL, payload, payload_cap);
    b.buf = payload; b.cap = payload_cap; b.pos = hdr_bits;
    bw_align(&b); /* byte_alignment() after the frame header inside OBU_FRAME */
    if (g.tile_cols * g.tile_rows > 1) {
      bw_put(&b, 0, 1); /* tile_start_and_end_present_flag */
      bw_align(&b);
    }
    pp = b.pos >> 3;
    for (tr = 0; tr < g.tile_rows; tr++)
      for (tc = 0; tc < g.tile_cols; tc++) {
        int last = tr == g.tile_rows - 1 && tc == g.tile_cols - 1;
        size_t n = encode_tile(e, tr, tc, tilebuf, payload_cap);
        if (n == (size_t)-1 || pp + n + 8 > payload_cap) goto done;
        if (!last) {
          uint32_t v = (uint32_t)(n - 1);
          payload[pp++] = (uint8_t)v; payload[pp++] = (uint8_t)(v >> 8);
          payload[pp++] = (uint8_t)(v >> 16); payload[pp++] = (uint8_t)(v >> 24);
        }
        memcpy(payload + pp, tilebuf, n);
        pp += n;
      }
    if (pos + 1 + (size_t)leb128_size(pp) + pp > out_cap) goto done;
    out[pos++] = (6 << 3) | 2; /* OBU_FRAME */
    pos += put_leb128(out + pos, pp);
    memcpy(out + pos, payload, pp);
    pos += pp;
  }
  /* CDEF -> final reconstruction */
  if (recon || stats) {
    Av1oFrame *fin = recon ? recon : av1o_frame_alloc(cfg->width, cfg->height);
    if (lr_out) { /* final reconstruction = loop-restored frame (decided in the first pass; the second is identical) */
      for (p = 0; p < 3; p++) {
        int pw = p ? cfg->width / 2 : cfg->width, ph = p ? cfg->height / 2 : cfg->height, y;
        for (y = 0; y < ph; y++) memcpy(fin->p[p] + (size_t)y * fin->stride[p], lr_out->p[p] + (size_t)y * lr_out->stride[p], sizeof(uint16_t) * (size_t)pw);
      }
    } else {
      int lv[4];
      av1o_deblock_levels(cfg, ref == NULL, lv);
      av1o_deblock_frame(cfg, e->rec, e->mi_bsl, e->mi_skip, e->mi_is_inter, g.mi_cols, lv, cfg->deblock == 2 ? cfg->lf_sharpness : 0);
      av1o_cdef_frame(cfg, e->rec, fin, e->mi_skip, g.mi_cols, e->cdef_idx_sb);
    }
    if (stats) {
      for (p = 0; p < 3; p++) {
        int pw = p ? cfg->width / 2 : cfg->width, ph = p ? cfg->height / 2 : cfg->height, x, y;
        uint64_t s = 0;
        for (y = 0; y < ph; y++)
          for (x = 0; x < pw; x++) {
            int d = (int)fin->p[p][y * fin->stride[p] + x] - (int)src->p[p][y * src->stride[p] + x];
            s += (uint64_t)(d * d);
          }
        stats->sse[p] = s;
      }
    }
    if (!recon) av1o_frame_free(fin);
  }
  ret = (long)pos;
done:
  free(payload);
  free(tilebuf);
  for (p = 0; p < 3; p++) { free(e->above_lvl[p]); free(e->above_dc[p]); }
  free(e->mi_bsl); free(e->mi_skip); free(e->mi_ymode); free(e->mi_uvmode); free(e->cdef_idx_sb);
  free(e->mi_is_inter); free(e->mi_newmv); free(e->mi_mv); free(e->me_centre);
  free(lr_units); av1o_frame_free(lr_out);
  av1o_frame_free(src_ext);
  av1o_frame_free(e->rec);
  free(e);
  return ret;
}
