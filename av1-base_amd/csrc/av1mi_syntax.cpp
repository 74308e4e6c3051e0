// av1mi_syntax.cpp - the host code that needs no GPU (av1mi_syntax.h): no HIP header, any host C++ compiler.
#include <string.h>

#include <cstddef>
#include <vector>

// The product build compiles every source as HIP, and the rule headers then mark their functions __host__ __device__ __forceinline__.
// The compiler knows the first two by itself; the third is a macro of the runtime's header, which this file does not include.
#if defined(__HIPCC__) && !defined(__forceinline__)
#define __forceinline__ inline __attribute__((always_inline))
#endif

#include "av1mi_syntax.h"
#include "av1_tables.h"
#include "lr_fit_rule.h"
#include "lr_rate_rule.h"
#include "deblock_pieces.h"
#include "aq_rule.h"
#include "tpl_rule.h"
#include "tf_rule.h"
#include "fg_rule.h"
#include "fg_denoise_rule.h"

namespace av1mi {

// ------------------------------------------------------------------ header bit writer
struct BitWriter {
  std::vector<uint8_t> buf;
  size_t bits = 0;
  void put(uint32_t v, int n) {
    for (int i = n - 1; i >= 0; i--) {
      if ((bits & 7) == 0) buf.push_back(0);
      buf.back() |= (uint8_t)(((v >> i) & 1) << (7 - (bits & 7)));
      bits++;
    }
  }
  void align() { while (bits & 7) put(0, 1); }
  void trailing() { put(1, 1); align(); }
  // ns(n), AV1 spec §4.10.7
  void put_ns(int n, int v) {
    int w = 0;
    while ((1 << w) <= n) w++;  // w = floor(log2 n) + 1
    int m = (1 << w) - n;
    if (v < m) put((uint32_t)v, w - 1);
    else { int x = v + m; put((uint32_t)(x >> 1), w - 1); put((uint32_t)(x & 1), 1); }
  }
};

static int tile_log2(int blk, int target) { int k = 0; while ((blk << k) < target) k++; return k; }
static int bits_for(unsigned v) { int n = 0; while (v) { n++; v >>= 1; } return n ? n : 1; }

static uint32_t recip32(uint32_t q) { return (uint32_t)((((uint64_t)1 << 32) + q - 1) / q); }
QuantSteps quant_steps(int qindex, int bit_depth) {
  const int dc = bit_depth == 8 ? av1_dc_q8[qindex] : av1_dc_q10[qindex], ac = bit_depth == 8 ? av1_ac_q8[qindex] : av1_ac_q10[qindex];
  return { dc, ac, recip32((uint32_t)dc), recip32((uint32_t)ac) };
}
static void set_quant_steps(Av1miDevParams &P, const QuantSteps &q) { P.dc_q = q.dc_q; P.ac_q = q.ac_q; P.dc_recip = q.dc_recip; P.ac_recip = q.ac_recip; }

// aom's quantizer_to_qindex[] (CQ level -> base_q_idx); 30 -> 120
const uint8_t kQuantizerToQindex[64] = {
  0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92, 96, 100, 104, 108, 112, 116, 120, 124,
  128, 132, 136, 140, 144, 148, 152, 156, 160, 164, 168, 172, 176, 180, 184, 188, 192, 196, 200, 204, 208, 212, 216, 220, 224, 228, 232, 236, 240, 244, 249, 255 };

int resolve(const av1mi_params *in, Resolved *r) {
  if (!in) return AV1MI_E_INVALID_ARG;
  r->p = *in;
  av1mi_params &p = r->p;
  if (p.width < 8 || p.height < 8 || (p.width & 1) || (p.height & 1) || p.width > 65536 || p.height > 65536) return AV1MI_E_INVALID_ARG;
  r->cw = (int)((p.width + 7) & ~7u); r->ch = (int)((p.height + 7) & ~7u);
  r->padded = r->cw != (int)p.width || r->ch != (int)p.height;
  if (p.bit_depth != 8 && p.bit_depth != 10) return AV1MI_E_INVALID_ARG;
  // cq_level 0 is base_q_idx 0: CodedLossless frames (spec 5.9.2), whose syntax this encoder does not write (no WHT, no lossless header)
  // ... and bits 8-10 of the field are the strength of the adaptive quantisation, 0 .. 4, bits 12-14 that of its temporal term, 0 .. 4;
  // bits 20-22 that of the frame term, 0 .. 4 (tpl_rule.h: every frame its own base_q_idx); nothing in bits 11, 15-19 or 23-31
  r->aq = (int)AV1MI_AQ_STRENGTH(p.cq_level);
  r->tpl = (int)AV1MI_TPL_STRENGTH(p.cq_level);
  r->fq = (int)AV1MI_FQ_STRENGTH(p.cq_level);
  if ((p.cq_level & ~0x7077FFu) || r->aq > AV1MI_AQ_MAX_STRENGTH || r->tpl > AV1MI_TPL_MAX_STRENGTH || r->fq > AV1MI_FQ_MAX_STRENGTH) return AV1MI_E_INVALID_ARG;
  p.cq_level = AV1MI_CQ_LEVEL(p.cq_level);
  if (p.cq_level == 0 || p.cq_level > 63) return AV1MI_E_INVALID_ARG;
  // film_grain bit 8 (AV1MI_FILM_GRAIN_ESTIMATE): the table is estimated from the chunk's source, the low byte N = 1 .. 50 its ceiling;
  // without it 0 .. 50 as ever.  Bit 10 with bit 8 (AV1MI_FILM_GRAIN_DENOISE): the source is denoised by that table before it is coded
  // (fg_denoise_rule.h).  Bits 12-13 with bit 8 (AV1MI_FILM_GRAIN_AR): the lag 1 .. 3 at which the grain's autoregressive coefficients are
  // fitted (fg_ar_rule.h).  Bits 14 and 15, both, with bits 8 and 10 (AV1MI_FILM_GRAIN_DENOISE_TEMPORAL): the denoiser's temporal term over
  // one neighbour each way, with bit 9 over two (fg_denoise_rule.h: av1mi_fgd_field_span).  Nothing in bit 11 or above bit 15, neither bit
  // 14 nor bit 15 alone, no bit 9 without them, and neither bit 10 nor bits 12-13 without bit 8
  r->fg_estimate = (p.film_grain & 0x100u) ? 1 : 0;
  r->fg_denoise = (p.film_grain & 0x400u) ? 1 : 0;
  r->fg_ar_lag = r->fg_estimate ? (int)AV1MI_FILM_GRAIN_AR_LAG(p.film_grain) : 0;
  r->fg_denoise_span = av1mi_fgd_field_span(p.film_grain);
  if (r->fg_denoise && !r->fg_estimate) return AV1MI_E_INVALID_ARG;
  if (((p.film_grain & 0xC000u) || (p.film_grain & 0x200u)) && !(r->fg_denoise_span && r->fg_denoise)) return AV1MI_E_INVALID_ARG;
  if (r->fg_estimate) {
    if ((p.film_grain & ~0xF7FFu) || (p.film_grain & 0xFFu) < 1 || (p.film_grain & 0xFFu) > AV1MI_FG_MAX_N) return AV1MI_E_INVALID_ARG;
    p.film_grain &= 0xFFu;
  }
  if (p.film_grain > AV1MI_FG_MAX_N) return AV1MI_E_INVALID_ARG;
  if (p.keyint == 0) p.keyint = 1;
  if (p.me_range == 0) p.me_range = 8;
  if (p.me_range != 8 && p.me_range != 16) return AV1MI_E_INVALID_ARG;
  if (p.block_log2 == 0) p.block_log2 = 5;
  if (p.block_log2 < 3 || p.block_log2 > 6) return AV1MI_E_INVALID_ARG;
  if (p.cdef_damping == 0) { p.cdef_y_pri = 2; p.cdef_y_sec = 0; p.cdef_uv_pri = 1; p.cdef_uv_sec = 0; p.cdef_damping = 5; }
  if (p.cdef_damping < 3 || p.cdef_damping > 6 || p.cdef_y_pri > 15 || p.cdef_uv_pri > 15 || p.cdef_y_sec > 3 || p.cdef_uv_sec > 3) return AV1MI_E_INVALID_ARG;
  if (p.cdef_search > 4 || (p.cdef_search && !p.enable_cdef)) return AV1MI_E_INVALID_ARG;
  if (p.deblock > 2) return AV1MI_E_INVALID_ARG;
  r->qidx = kQuantizerToQindex[p.cq_level];
  r->q = quant_steps(r->qidx, (int)p.bit_depth);
  // enable_lr bits 14 and 15, both (AV1MI_LR_RD): the rate term, with any low byte 1 .. 4, either fit and a unit size; bits 9 and 11 are
  // then its scale.  lambda stays with base_q_idx under adaptive quantisation, like the deblocking level.  (Without both bits the four
  // stay in the field, which the checks below refuse.)
  r->lr_lambda = 0;
  if (AV1MI_LR_RD_ON(p.enable_lr)) {
    const uint32_t low = p.enable_lr & 0xFFu;
    if (low < 1 || low > 4) return AV1MI_E_INVALID_ARG;
    r->lr_lambda = (uint32_t)av1mi_lr_lambda_of_step((unsigned long long)r->q.dc_q, (int)AV1MI_LR_RD_SCALE(p.enable_lr));
    p.enable_lr &= ~0xCA00u;
  }
  // enable_lr bits 12-13 (AV1MI_LR_UNIT_128 / _256): the unit size, with any low byte 1 .. 4 and either fit; 3 is no size
  r->lr_unit_shift = (int)((p.enable_lr >> 12) & 3u);
  if (r->lr_unit_shift) {
    const uint32_t low = p.enable_lr & 0xFFu;
    if (r->lr_unit_shift > AV1MI_LR_MAX_UNIT_SHIFT || low < 1 || low > 4) return AV1MI_E_INVALID_ARG;
    p.enable_lr &= ~0x3000u;
  }
  // enable_lr bit 8 (AV1MI_LR_FIT): the self-guided fit on switchable units, bits 16-31 the sets searched (0 = all); nothing else in bits 9-15
  // bit 10 (AV1MI_LR_WIENER_FIT): the Wiener fit, with any low byte 1 .. 4, alone or with bit 8
  r->lr_fit_mask = 0;
  r->lr_wfit = 0;
  if (p.enable_lr & 0x400u) {
    const uint32_t low = p.enable_lr & 0xFFu;
    if (low < 1 || low > 4 || (p.enable_lr & 0xFA00u) || (!(p.enable_lr & 0x100u) && (p.enable_lr >> 16))) return AV1MI_E_INVALID_ARG;
    r->lr_wfit = 1;
    p.enable_lr &= ~0x400u;
  }
  if (p.enable_lr & 0x100u) {
    const uint32_t low = p.enable_lr & 0xFFu;
    if ((p.enable_lr & 0xFE00u) || (low != 2 && low != 4)) return AV1MI_E_INVALID_ARG;
    r->lr_fit_mask = (p.enable_lr >> 16) ? (p.enable_lr >> 16) : 0xFFFFu;
    p.enable_lr = low;
  }
  if (p.subpel > 1 || p.enable_lr > 4 || p.color_range > 1 || p.intra_angle_delta > 1 || p.intra_edge_filter > 1 || p.cfl > 1 || p.tx_search > 1) return AV1MI_E_INVALID_ARG;
  if (p.partition_search > 2 || !av1mi_tf_field_ok(p.me_presearch)) return AV1MI_E_INVALID_ARG;
  // me_presearch bits 8-10 and 12-14 (AV1MI_ME_TF): the temporal filter's followers and strength; bit 0 stays as the pre-search's switch
  r->tf_frames = av1mi_tf_field_frames(p.me_presearch); r->tf_strength = av1mi_tf_field_strength(p.me_presearch);
  p.me_presearch = (uint32_t)av1mi_tf_field_presearch(p.me_presearch);
  // enable_lr 3 / 4 = 1 / 2 on all three planes: the frames' restoration type plus the chroma flag
  r->lr_chroma = p.enable_lr >= 3;
  if (r->lr_chroma) p.enable_lr -= 2;
  if (p.min_block_log2 == 0) p.min_block_log2 = 3;
  if (p.min_block_log2 < 3 || p.min_block_log2 > p.block_log2) return AV1MI_E_INVALID_ARG;
  if (p.color_primaries > 255 || p.transfer_characteristics > 255 || p.matrix_coefficients > 255) return AV1MI_E_INVALID_ARG;
  // CP_BT_709 / TC_SRGB / MC_IDENTITY switches the syntax to 4:4:4 with no color_range bit (spec 5.5.2): not a 4:2:0 description
  if (p.color_primaries == 1 && p.transfer_characteristics == 13 && p.matrix_coefficients == 0) return AV1MI_E_INVALID_ARG;
  if (p.enable_qm > 1 || p.qm_min > 15 || p.qm_max > 15 || (p.enable_qm && p.qm_min > p.qm_max)) return AV1MI_E_INVALID_ARG;
  // level from the quantiser index, as SVT-AV1 / libaom derive it ("--qm-min", "--qm-max")
  r->qm_level = p.enable_qm ? (int)(p.qm_min + (uint32_t)r->qidx * (p.qm_max + 1 - p.qm_min) / 256) : 15;
  r->sb_cols = (r->cw + 63) / 64;
  r->sb_rows = (r->ch + 63) / 64;
  // AV1 allows at most 64 x 64 tiles: frames beyond 64 superblocks either way (8K) use tiles of 2 x 2 superblocks
  if (p.tile_sb > 2) return AV1MI_E_INVALID_ARG;
  r->tile_sb = p.tile_sb ? (int)p.tile_sb : ((r->sb_cols > 64 || r->sb_rows > 64) ? 2 : 1);
  r->tile_cols = (r->sb_cols + r->tile_sb - 1) / r->tile_sb;
  r->tile_rows = (r->sb_rows + r->tile_sb - 1) / r->tile_sb;
  if (r->tile_cols > 64 || r->tile_rows > 64) return AV1MI_E_UNSUPPORTED;
  return AV1MI_OK;
}

// deblocking level of a frame (the same for all four filters): libaom's "pick from q" rule; 0 = filter off
static int deblock_level(const Resolved &r, bool key) {
  if (!r.p.deblock) return 0;
  int g = r.p.bit_depth == 8 ? (r.q.ac_q * 20723 + 1015158) >> 18 : (r.q.ac_q * 20723 + 4060632) >> 20;
  if (key) g -= 4;
  return g < 0 ? 0 : (g > 63 ? 63 : g);
}

// bytes of n frames in the caller's layout: tight at the signalled size (the coded size, where that is a multiple of 8 both ways).
// Width and height are even (resolve), so a frame's 3 / 2 is exact and multiplying by n first changes nothing.
size_t caller_bytes(const Resolved &r, size_t n) { return n * r.p.width * r.p.height * 3 / 2 * (r.p.bit_depth > 8 ? 2 : 1); }

// sequence_header_obu (AV1 spec §5.5), complete OBU incl. header and size
std::vector<uint8_t> make_sequence_header(const Resolved &r) {
  const av1mi_params &p = r.p;
  BitWriter b;
  const int wbits = bits_for(p.width - 1), hbits = bits_for(p.height - 1);
  b.put(0, 3);   // seq_profile
  b.put(0, 1);   // still_picture
  b.put(0, 1);   // reduced_still_picture_header
  b.put(0, 1);   // timing_info_present_flag
  b.put(0, 1);   // initial_display_delay_present_flag
  b.put(0, 5);   // operating_points_cnt_minus_1
  b.put(0, 12);  // operating_point_idc[0]
  b.put(31, 5);  // seq_level_idx[0]: maximum parameters
  b.put(0, 1);   // seq_tier[0]
  b.put((uint32_t)(wbits - 1), 4);
  b.put((uint32_t)(hbits - 1), 4);
  b.put(p.width - 1, wbits);
  b.put(p.height - 1, hbits);
  b.put(0, 1);  // frame_id_numbers_present_flag
  b.put(0, 1);  // use_128x128_superblock
  b.put(0, 1);  // enable_filter_intra
  b.put(p.intra_edge_filter ? 1 : 0, 1);  // enable_intra_edge_filter
  b.put(0, 1);  // enable_interintra_compound
  b.put(0, 1);  // enable_masked_compound
  b.put(0, 1);  // enable_warped_motion
  b.put(0, 1);  // enable_dual_filter
  b.put(0, 1);  // enable_order_hint
  b.put(0, 1);  // seq_choose_screen_content_tools
  b.put(0, 1);  // seq_force_screen_content_tools
  b.put(0, 1);  // enable_superres
  b.put(p.enable_cdef ? 1 : 0, 1);
  b.put(p.enable_lr ? 1 : 0, 1);  // enable_restoration
  // color_config
  b.put(p.bit_depth > 8, 1);  // high_bitdepth
  b.put(0, 1);                // mono_chrome
  {
    const bool desc = p.color_primaries || p.transfer_characteristics || p.matrix_coefficients;
    b.put(desc, 1);           // color_description_present_flag (absent: CP / TC / MC = 2 "unspecified")
    // a partial triple: each field left at 0 is written as 2 "unspecified" (0 is a reserved primaries / transfer code, and MC 0 =
    // MC_IDENTITY is not allowed with 4:2:0, spec 5.5.2); the Matroska Colour element maps 0 the same way
    auto code = [](uint32_t v) { return v ? v : 2u; };
    if (desc) { b.put(code(p.color_primaries), 8); b.put(code(p.transfer_characteristics), 8); b.put(code(p.matrix_coefficients), 8); }
  }
  b.put(p.color_range ? 1 : 0, 1);  // color_range: 0 = studio (limited) range, 1 = full range
  b.put(0, 2);                // chroma_sample_position
  b.put(0, 1);                // separate_uv_delta_q
  b.put(p.film_grain ? 1 : 0, 1);  // film_grain_params_present
  b.trailing();
  std::vector<uint8_t> out;
  out.push_back((1 << 3) | 2);
  out.push_back((uint8_t)b.buf.size());  // < 128
  out.insert(out.end(), b.buf.begin(), b.buf.end());
  return out;
}

// OBU_FRAME payload up to the first tile: frame_header_obu (§5.9) + byte_alignment +
// tile_group_obu's tile_start_and_end_present_flag + byte_alignment (§5.11.1)
// cdef_str_bit (optional): bit offset of the first CDEF strength field - with the search on (cdef_bits > 0) the header carries the fixed
// strengths as placeholders, 2^cdef_bits times, and cdef_select_kernel overwrites those 12 * 2^cdef_bits bits in the frame's slot
// lf_bit (optional): bit offset of loop_filter_level[0] - with the level search on (deblock = 2) the header carries the pool's D = 0
// entries as placeholders, max(g, 1), max(g, 1), g, g, and deblock_decide_kernel overwrites those 24 bits in the frame's slot (luma
// never picks 0, so all four fields are coded whatever is chosen)
// fg_bit (optional): bit offset of the first luma point of film_grain_params - with the estimate on (film_grain bit 8) the table has eight
// points per plane at x = 16 + 32 k (fg_rule.h) whose values the header carries at the ceiling, 2 N luma / N chroma, as placeholders, and
// fg_table_kernel overwrites those 24 values in every frame's slot
// fg_ar_bit (optional): bit offset of the first luma coefficient - with a lag L (film_grain bits 12-13) the header carries ar_coeff_lag = L
// and 2 L (L + 1) luma, then 2 L (L + 1) + 1 cb and as many cr coefficients as 128 (zero) placeholders, 6 L (L + 1) + 2 bytes in a row
// which fg_ar_solve_kernel overwrites in every frame's slot, with the points scaled by the fit's gain; ar_coeff_shift_minus_6 is then 1
// q_bit (optional): bit offset of base_q_idx - with the frame term on (cq_level bits 20-22) the header carries the chunk's index as the
// placeholder and aq_map_kernel overwrites those 8 bits with the frame's q_f in its slot (the field is not byte-aligned)
std::vector<uint8_t> make_frame_header(const Resolved &r, size_t *hdr_bits, uint32_t frame_number, bool inter, size_t *cdef_str_bit, size_t *lf_bit,
                                       size_t *fg_bit, size_t *fg_ar_bit, size_t *q_bit) {
  const av1mi_params &p = r.p;
  BitWriter b;
  b.put(0, 1);  // show_existing_frame
  b.put(inter ? 1 : 0, 2);  // frame_type KEY_FRAME / INTER_FRAME
  b.put(1, 1);  // show_frame
  if (inter) b.put(0, 1);  // error_resilient_mode (implied 1 on shown key frames)
  b.put(p.cdf_update ? 0 : 1, 1);  // disable_cdf_update
  b.put(0, 1);  // frame_size_override_flag
  if (inter) {
    b.put(7, 3);     // primary_ref_frame = NONE: every frame starts from the default CDFs (tiles of all frames stay independent)
    b.put(0x01, 8);  // refresh_frame_flags: this frame replaces slot 0
    for (int i = 0; i < 7; i++) b.put(0, 3);  // ref_frame_idx[i] = 0: every reference name -> the previous frame
  }
  b.put(0, 1);  // render_and_frame_size_different
  if (inter) {
    b.put(0, 1);  // allow_high_precision_mv
    b.put(0, 1);  // is_filter_switchable
    b.put(r.p.subpel ? 0 : 3, 2);  // interpolation_filter: EIGHTTAP with sub-sample vectors, else BILINEAR
    b.put(0, 1);  // is_motion_mode_switchable
  }
  if (p.cdf_update) b.put(1, 1);  // disable_frame_end_update_cdf
  // tile_info (§5.9.15): explicit spacing, tiles of tile_sb x tile_sb superblocks (the last row/column may be short)
  {
    const int sb_cols = r.sb_cols, sb_rows = r.sb_rows, ts = r.tile_sb;
    const int max_tile_width_sb = 4096 >> 6, max_tile_area_sb = (4096 * 2304) >> 12;
    int min_log2_tile_cols = tile_log2(max_tile_width_sb, sb_cols);
    int min_log2_tiles = tile_log2(max_tile_area_sb, sb_rows * sb_cols);
    if (min_log2_tiles < min_log2_tile_cols) min_log2_tiles = min_log2_tile_cols;
    b.put(0, 1);  // uniform_tile_spacing_flag
    int widest = 0;
    for (int start = 0; start < sb_cols; start += ts) {
      const int max_w = sb_cols - start < max_tile_width_sb ? sb_cols - start : max_tile_width_sb;
      const int sz = sb_cols - start < ts ? sb_cols - start : ts;
      b.put_ns(max_w, sz - 1);  // width_in_sbs_minus_1
      if (sz > widest) widest = sz;
    }
    int area = sb_rows * sb_cols;
    if (min_log2_tiles > 0) area >>= (min_log2_tiles + 1);
    int max_tile_height_sb = area / widest;
    if (max_tile_height_sb < 1) max_tile_height_sb = 1;
    for (int start = 0; start < sb_rows; start += ts) {
      const int max_h = sb_rows - start < max_tile_height_sb ? sb_rows - start : max_tile_height_sb;
      const int sz = sb_rows - start < ts ? sb_rows - start : ts;
      b.put_ns(max_h, sz - 1);  // height_in_sbs_minus_1
    }
    const int cl = tile_log2(1, r.tile_cols), rl = tile_log2(1, r.tile_rows);
    if (cl > 0 || rl > 0) {
      b.put(0, cl + rl);  // context_update_tile_id
      b.put(3, 2);        // tile_size_bytes_minus_1
    }
  }
  if (q_bit) *q_bit = b.bits;
  b.put((uint32_t)r.qidx, 8);  // base_q_idx
  b.put(0, 1);  // DeltaQYDc
  b.put(0, 1);  // DeltaQUDc
  b.put(0, 1);  // DeltaQUAc
  b.put(r.p.enable_qm ? 1 : 0, 1);  // using_qmatrix
  if (r.p.enable_qm) { b.put((uint32_t)r.qm_level, 4); b.put((uint32_t)r.qm_level, 4); }  // qm_y, qm_u (= qm_v: separate_uv_delta_q = 0)
  b.put(0, 1);  // segmentation_enabled
  if (r.qidx > 0) b.put(dq_on(r) ? 1 : 0, 1);  // delta_q_present
  if (dq_on(r)) {
    b.put(2, 2);  // delta_q_res: deltas in steps of 4
    b.put(0, 1);  // delta_lf_present
  }
  {  // loop_filter_params (§5.9.11): level 0 = deblocking off
    const uint32_t lv = (uint32_t)deblock_level(r, !inter), ly = p.deblock == 2 ? (uint32_t)av1mi_lf_pool((int)lv, 7, 0) : lv;
    if (lf_bit) *lf_bit = b.bits;
    b.put(ly, 6); b.put(ly, 6);          // loop_filter_level[0..1]
    if (ly) { b.put(lv, 6); b.put(lv, 6); }  // [2..3] (U, V)
  }
  b.put(0, 3);  // loop_filter_sharpness
  b.put(0, 1);  // loop_filter_delta_enabled
  if (p.enable_cdef) {
    b.put(p.cdef_damping - 3, 2);
    const int cdef_bits = p.cdef_search ? (int)p.cdef_search - 1 : 0;
    b.put((uint32_t)cdef_bits, 2);
    if (cdef_str_bit) *cdef_str_bit = b.bits;
    for (int i = 0; i < (1 << cdef_bits); i++) {
      b.put(p.cdef_y_pri, 4); b.put(p.cdef_y_sec, 2);
      b.put(p.cdef_uv_pri, 4); b.put(p.cdef_uv_sec, 2);
    }
  }
  if (p.enable_lr) {  // lr_params (§5.9.20): lr_type per plane, then the unit size: lr_unit_shift 0 = 64x64 luma units, 1 = 128x128 or,
                      // with lr_unit_extra_shift, 256x256
    const uint32_t t = p.enable_lr == 2 ? 1 : 2;  // lr_type: 1 = RESTORE_SWITCHABLE, 2 = RESTORE_WIENER
    b.put(t, 2); b.put(r.lr_chroma ? t : 0, 2); b.put(r.lr_chroma ? t : 0, 2);  // Y, U, V: chroma the luma type with enable_lr 3 / 4
    b.put(r.lr_unit_shift > 0 ? 1 : 0, 1);                          // lr_unit_shift (the superblocks are 64x64)
    if (r.lr_unit_shift) b.put(r.lr_unit_shift == 2 ? 1 : 0, 1);    // lr_unit_extra_shift
    if (r.lr_chroma) b.put(1, 1);  // lr_uv_shift: chroma units of half the luma size, the picture area of a luma unit
  }
  b.put(0, 1);  // tx_mode_select = 0: TX_MODE_LARGEST
  if (inter) b.put(0, 1);  // reference_select = 0
  b.put(0, 1);  // reduced_tx_set
  if (inter) for (int i = 0; i < 7; i++) b.put(0, 1);  // global_motion_params: is_global = 0
  if (p.film_grain) {  // film_grain_params (§5.9.30): fixed table, per-frame seed
    const uint32_t sy = p.film_grain * 2 > 255 ? 255 : p.film_grain * 2, sc = p.film_grain;
    b.put(1, 1);                                              // apply_grain
    b.put((7391u + 173u * (p.first_frame + frame_number)) & 0xFFFFu, 16);  // grain_seed
    if (inter) b.put(1, 1);                                   // update_grain (implied on key frames)
    if (r.fg_estimate) {                                      // eight points per plane, the ceiling as placeholders
      b.put(AV1MI_FG_BINS, 4);                                // num_y_points
      if (fg_bit) *fg_bit = b.bits;
      for (int k = 0; k < AV1MI_FG_BINS; k++) { b.put((uint32_t)av1mi_fg_point_x(k), 8); b.put(sy, 8); }
      b.put(0, 1);                                            // chroma_scaling_from_luma
      for (int pl = 0; pl < 2; pl++) {
        b.put(AV1MI_FG_BINS, 4);                              // num_cb_points, num_cr_points
        for (int k = 0; k < AV1MI_FG_BINS; k++) { b.put((uint32_t)av1mi_fg_point_x(k), 8); b.put(sc, 8); }
      }
    } else {
      b.put(2, 4); b.put(0, 8); b.put(sy, 8); b.put(255, 8); b.put(sy, 8);  // num_y_points + points
      b.put(0, 1);                                              // chroma_scaling_from_luma
      for (int pl = 0; pl < 2; pl++) { b.put(2, 4); b.put(0, 8); b.put(sc, 8); b.put(255, 8); b.put(sc, 8); }
    }
    b.put(3, 2);                                              // grain_scaling_minus_8
    const int lag = r.fg_ar_lag, n_pos = 2 * lag * (lag + 1);
    b.put((uint32_t)lag, 2);                                  // ar_coeff_lag
    if (fg_ar_bit) *fg_ar_bit = lag ? b.bits : 0;
    for (int i = 0; i < n_pos; i++) b.put(128, 8);            // ar_coeffs_y_plus_128 (there are luma points whenever there is a lag)
    for (int i = 0; i < 2 * (n_pos + 1); i++) b.put(128, 8);  // ar_coeffs_cb/cr_plus_128: the positions and the luma tap
    b.put(lag ? 1 : 0, 2);                                    // ar_coeff_shift_minus_6: Q7 coefficients with a lag
    b.put(0, 2);                                              // grain_scale_shift
    for (int pl = 0; pl < 2; pl++) { b.put(128, 8); b.put(192, 8); b.put(256, 9); }  // mult, luma_mult, offset
    b.put(1, 1);                                              // overlap_flag
    b.put(0, 1);                                              // clip_to_restricted_range
  }
  if (hdr_bits) *hdr_bits = b.bits;
  b.align();
  if (r.tile_cols * r.tile_rows > 1) { b.put(0, 1); b.align(); }  // tile_start_and_end_present_flag
  return b.buf;
}

// ---- loop restoration unit syntax (§5.11.58): the literal bits that code a Wiener coefficient set against the
// tile-start reference Wiener_Taps_Mid = {3, -7, 15} (tiles are one superblock = one unit, so that is always the
// reference).  The writers (lr_put_signed_ref and what it calls, av1mi_lr_sgr_code) are lr_fit_rule.h's: the self-guided
// fit runs them on the device, and the fixed candidates' constant strings below come from the same functions.
using BitString = Av1miBitString;
// (the fixed candidates - av1mi_wiener_cand, av1mi_wiener_cand_uv, av1mi_sgr_cand - are lr_fit_rule.h's, which the kernels read as well)
// self-guided unit (§5.11.58): lr_sgr_set L(4), then the two weights against RefSgrXqd (ref 0 = Sgrproj_Xqd_Mid at the tile
// start, r = candidate r-1: the previous self-guided unit of the tile).  Every candidate uses set 9, whose radii are both
// non-zero, so both weights are always coded.
static BitString sgr_code_of(int ref, int cand) {
  static const int mid[2] = { -32, 31 };
  return av1mi_lr_sgr_code(av1mi_sgr_cand[cand][0], av1mi_sgr_cand[cand][1], av1mi_sgr_cand[cand][2], ref ? av1mi_sgr_cand[ref - 1][1] : mid[0], ref ? av1mi_sgr_cand[ref - 1][2] : mid[1]);
}
// ref: 0 = Wiener_Taps_Mid (tile start), r = candidate r-1 (the previous unit of the tile that was coded with a filter)
static BitString lr_code_of(int ref, int cand) {
  static const int tmin[3] = { -5, -23, -17 }, tmax[3] = { 10, 8, 46 }, tk[3] = { 1, 2, 3 }, mid[3] = { 3, -7, 15 };
  BitString b;
  for (int pass = 0; pass < 2; pass++)
    for (int j = 0; j < 3; j++) lr_put_signed_ref(b, tmin[j], tmax[j] + 1, tk[j], ref ? av1mi_wiener_cand[ref - 1][j] : mid[j], av1mi_wiener_cand[cand][j]);
  return b;
}
// the same for a chroma unit: taps 1 and 2 of each pass, against the plane's RefLrWiener
static BitString lr_code_of_uv(int ref, int cand) {
  static const int tmin[3] = { -5, -23, -17 }, tmax[3] = { 10, 8, 46 }, tk[3] = { 1, 2, 3 }, mid[3] = { 3, -7, 15 };
  BitString b;
  for (int pass = 0; pass < 2; pass++)
    for (int j = 1; j < 3; j++) lr_put_signed_ref(b, tmin[j], tmax[j] + 1, tk[j], ref ? av1mi_wiener_cand_uv[ref - 1][j] : mid[j], av1mi_wiener_cand_uv[cand][j]);
  return b;
}

// default CDF blob for one q context in the layout of Av1miCdfLayout (inverted, 0, counter)
template <size_t W>
static void emit_rows(std::vector<uint16_t> &v, size_t off, const uint16_t (*rows)[W], int nrows, int row_stride, const int *nsym, int nsym_const) {
  for (int i = 0; i < nrows; i++) {
    int n = nsym ? nsym[i] : nsym_const;
    for (int k = 0; k < n - 1; k++) v[off + (size_t)i * row_stride + k] = (uint16_t)(32768 - rows[i][k]);
  }
}
std::vector<uint16_t> make_cdf_blob(int qidx) {
  typedef Av1miCdfLayout CL;
  const int q = av1mi_q_context(qidx);
  std::vector<uint16_t> v(CL::TOTAL, 0);
  int pn[20];
  for (int i = 0; i < 20; i++) pn[i] = i < 4 ? 4 : (i < 16 ? 10 : 8);
  emit_rows(v, CL::PARTITION, av1_default_partition_cdf, 16, 11, pn, 0);
  emit_rows(v, CL::KF_Y_MODE, &av1_default_kf_y_mode_cdf[0][0], 25, 14, nullptr, 13);
  emit_rows(v, CL::UV_MODE, av1_default_uv_mode_nocfl_cdf, 13, 15, nullptr, 13);
  emit_rows(v, CL::UV_MODE + 13 * 15, av1_default_uv_mode_cfl_cdf, 13, 15, nullptr, 14);
  emit_rows(v, CL::ANGLE_DELTA, av1_default_angle_delta_cdf, 8, 8, nullptr, 7);
  emit_rows(v, CL::SKIP, av1_default_skip_cdf, 3, 3, nullptr, 2);
  emit_rows(v, CL::TX_SET1, &av1_default_intra_tx_set1_cdf[0][0], 26, 8, nullptr, 7);
  emit_rows(v, CL::TX_SET2, &av1_default_intra_tx_set2_cdf[0][0], 39, 6, nullptr, 5);
  emit_rows(v, CL::TXB_SKIP, &av1_default_txb_skip_cdf[q][0][0], 65, 3, nullptr, 2);
  emit_rows(v, CL::EOB16, &av1_default_eob_multi16_cdf[q][0][0], 4, 6, nullptr, 5);
  emit_rows(v, CL::EOB32, &av1_default_eob_multi32_cdf[q][0][0], 4, 7, nullptr, 6);
  emit_rows(v, CL::EOB64, &av1_default_eob_multi64_cdf[q][0][0], 4, 8, nullptr, 7);
  emit_rows(v, CL::EOB128, &av1_default_eob_multi128_cdf[q][0][0], 4, 9, nullptr, 8);
  emit_rows(v, CL::EOB256, &av1_default_eob_multi256_cdf[q][0][0], 4, 10, nullptr, 9);
  emit_rows(v, CL::EOB512, &av1_default_eob_multi512_cdf[q][0][0], 4, 11, nullptr, 10);
  emit_rows(v, CL::EOB1024, &av1_default_eob_multi1024_cdf[q][0][0], 4, 12, nullptr, 11);
  emit_rows(v, CL::EOB_EXTRA, &av1_default_eob_extra_cdf[q][0][0][0], 90, 3, nullptr, 2);
  emit_rows(v, CL::DC_SIGN, &av1_default_dc_sign_cdf[q][0][0], 6, 3, nullptr, 2);
  emit_rows(v, CL::COEFF_BASE_EOB, &av1_default_coeff_base_eob_cdf[q][0][0][0], 40, 4, nullptr, 3);
  emit_rows(v, CL::USE_WIENER, av1_default_use_wiener_cdf, 1, 3, nullptr, 2);
  emit_rows(v, CL::RESTORE_SW, av1_default_switchable_restore_cdf, 1, 4, nullptr, 3);
  emit_rows(v, CL::CFL_SIGN, av1_default_cfl_sign_cdf, 1, 9, nullptr, 8);
  emit_rows(v, CL::CFL_ALPHA, av1_default_cfl_alpha_cdf, 6, 17, nullptr, 16);
  emit_rows(v, CL::DELTA_Q, av1_default_delta_q_cdf, 1, 5, nullptr, 4);
  // inter frames
  emit_rows(v, CL::IF_Y_MODE, av1_default_if_y_mode_cdf, 4, 14, nullptr, 13);
  emit_rows(v, CL::IS_INTER, av1_default_is_inter_cdf, 4, 3, nullptr, 2);
  emit_rows(v, CL::NEWMV, av1_default_newmv_cdf, 6, 3, nullptr, 2);
  emit_rows(v, CL::GLOBALMV, av1_default_globalmv_cdf, 2, 3, nullptr, 2);
  emit_rows(v, CL::REFMV, av1_default_refmv_cdf, 6, 3, nullptr, 2);
  emit_rows(v, CL::DRL, av1_default_drl_cdf, 3, 3, nullptr, 2);
  emit_rows(v, CL::SINGLE_REF, &av1_default_single_ref_cdf[0][0], 18, 3, nullptr, 2);
  emit_rows(v, CL::INTER_TX1, av1_default_inter_tx_set1_cdf, 2, 17, nullptr, 16);
  emit_rows(v, CL::INTER_TX2, av1_default_inter_tx_set2_cdf, 1, 13, nullptr, 12);
  emit_rows(v, CL::INTER_TX3, av1_default_inter_tx_set3_cdf, 4, 3, nullptr, 2);
  emit_rows(v, CL::MV_JOINT, av1_default_mv_joint_cdf, 1, 5, nullptr, 4);
  for (int c = 0; c < 2; c++) {
    const size_t b0 = CL::MV_COMP + (size_t)c * CL::MVC_SIZE;
    emit_rows(v, b0 + CL::MVC_CLASS, av1_default_mv_class_cdf, 1, 12, nullptr, 11);
    emit_rows(v, b0 + CL::MVC_CLASS0_FP, av1_default_mv_class0_fp_cdf, 2, 5, nullptr, 4);
    emit_rows(v, b0 + CL::MVC_FP, av1_default_mv_fp_cdf, 1, 5, nullptr, 4);
    emit_rows(v, b0 + CL::MVC_SIGN, av1_default_mv_sign_cdf, 1, 3, nullptr, 2);
    emit_rows(v, b0 + CL::MVC_CLASS0_HP, av1_default_mv_class0_hp_cdf, 1, 3, nullptr, 2);
    emit_rows(v, b0 + CL::MVC_HP, av1_default_mv_hp_cdf, 1, 3, nullptr, 2);
    emit_rows(v, b0 + CL::MVC_CLASS0, av1_default_mv_class0_cdf, 1, 3, nullptr, 2);
    emit_rows(v, b0 + CL::MVC_BITS, av1_default_mv_bits_cdf, 10, 3, nullptr, 2);
  }
  emit_rows(v, CL::COEFF_BASE, &av1_default_coeff_base_cdf[q][0][0][0], 420, 5, nullptr, 4);
  emit_rows(v, CL::COEFF_BR, &av1_default_coeff_br_cdf[q][0][0][0], 210, 5, nullptr, 4);
  return v;
}

// Per-tile capacities (per superblock of the tile): 8192 symbol-stream entries and 4096 output bytes hold any tile of
// ordinary content down to about CQ 20 (1080p clip at CQ 30: longest tile 4826 entries, ~1.2 KB); a tile that outgrows
// them is detected on the device and the chunk is re-run at the next multiplier, which the context then keeps.
// x32 / x64 reach the true worst case of a 64x64 4:2:0 tile (6144 coefficients x <= 37 stream entries: base + 4
// range + sign + 31 Golomb bits; <= 10 output bytes per coefficient), so the retry ends.
int tile_slot_bytes(const Resolved &r, int scale) { return 4096 * scale * r.tile_sb * r.tile_sb; }
int tile_stream_cap(const Resolved &r, int scale) { return 8192 * scale * r.tile_sb * r.tile_sb; }

// the self-guided fit's units of a chunk - its frames' restoration units over three planes - and the bytes of their block
size_t fit_chunk_units(const Resolved &r, size_t n_frames) {
  return n_frames * 3 * (size_t)av1mi_lr_count((int)r.p.height, r.lr_unit_shift) * (size_t)av1mi_lr_count((int)r.p.width, r.lr_unit_shift);
}

// the temporal filter's keys of a chunk: [key frame][follower 1 .. tf_frames][16x16 block of the coded size]
size_t tf_mv_entries(const Resolved &r, size_t n_frames) {
  return (size_t)av1mi_tf_key_frames((int)r.p.keyint, (int)n_frames) * (size_t)r.tf_frames * (size_t)av1mi_tf_blocks(r.cw) * (size_t)av1mi_tf_blocks(r.ch);
}
// the film-grain denoiser's temporal keys of a chunk: [frame][slot g - f = -2, -1, +1, +2][16x16 block of the coded size]
size_t fgd_mv_entries(const Resolved &r, size_t n_frames) {
  return n_frames * AV1MI_FGD_SLOTS * (size_t)av1mi_tf_blocks(r.cw) * (size_t)av1mi_tf_blocks(r.ch);
}
// whether the filter changes any frame of the chunk: some key frame has a follower (its first key frame then has)
bool tf_runs(const Resolved &r, size_t n_frames) { return av1mi_tf_followers(r.tf_frames, (int)r.p.keyint, (int)n_frames, 0) > 0; }

// The kernels' parameters of a chunk of `n_frames` frames: `r` at the coded size and the per-tile capacities of multiplier `scale`.
// Every buffer pointer stays null (memset): bind_workspace binds a chunk's, a stand-alone pass hands its kernels their buffers directly.
// The header sizes follow with the headers (prepare_chunk).
Av1miDevParams dev_params(const Resolved &r, uint32_t n_frames, int scale) {
  const av1mi_params &p = r.p;
  Av1miDevParams P;
  memset(&P, 0, sizeof(P));
  P.width = r.cw; P.height = r.ch; P.bit_depth = p.bit_depth; P.true_w = (int)p.width; P.true_h = (int)p.height;
  P.mi_rows = r.ch / 4; P.mi_cols = r.cw / 4; P.b8_rows = r.ch / 8; P.b8_cols = r.cw / 8; P.sb_rows = r.sb_rows; P.sb_cols = r.sb_cols;
  P.tile_sb = r.tile_sb; P.tile_rows = r.tile_rows; P.tile_cols = r.tile_cols;
  P.n_frames = (int)n_frames;
  P.base_q_idx = r.qidx;
  P.qctx = av1mi_q_context(r.qidx);
  set_quant_steps(P, r.q);
  P.using_qm = p.enable_qm ? 1 : 0; P.qm_y = P.qm_uv = r.qm_level;
  P.max_bs_log2 = (int)p.block_log2;
  P.min_bs_log2 = p.partition_search ? (int)p.min_block_log2 : (int)p.block_log2;
  P.mode_mask = p.intra_mode_mask ? (p.intra_mode_mask & 0x1FFF) : 0x0007;  // default candidates: DC, V, H
  P.angle_delta = p.intra_angle_delta ? 1 : 0; P.edge_filter = p.intra_edge_filter ? 1 : 0; P.cfl = p.cfl ? 1 : 0; P.tx_search = p.tx_search ? 1 : 0;
  P.enable_cdef = p.enable_cdef ? 1 : 0;
  P.cdef_y_pri = p.cdef_y_pri; P.cdef_y_sec = p.cdef_y_sec; P.cdef_uv_pri = p.cdef_uv_pri; P.cdef_uv_sec = p.cdef_uv_sec;
  P.cdef_damping = p.cdef_damping; P.cdef_search = (int)p.cdef_search;
  if (p.cdef_search) P.cdef_bits = (int)p.cdef_search - 1;
  P.disable_cdf_update = p.cdf_update ? 0 : 1;
  P.stride_y = r.cw; P.stride_c = r.cw / 2; P.frame_samples = (long)r.cw * r.ch * 3 / 2;
  P.plane_off_u = (long)r.cw * r.ch; P.plane_off_v = P.plane_off_u + (long)(r.cw / 2) * (r.ch / 2);
  P.tile_slot_bytes = tile_slot_bytes(r, scale); P.stream_cap = tile_stream_cap(r, scale); P.tile_size_bytes = 4;
  P.keyint = (int)p.keyint; P.me_range = (int)p.me_range; P.subpel = p.subpel ? 1 : 0; P.me_presearch = p.me_presearch ? 1 : 0;
  P.hdr_slot_bytes = 512;
  for (int i = 0; i < 4; i++) { P.lf_level[i] = deblock_level(r, true); P.lf_level_inter[i] = deblock_level(r, false); }
  if (p.deblock == 2) {   // the level search: the header's placeholders (luma at least 1: every frame is deblocked)
    P.lf_search = 1;
    P.lf_search_g[0] = P.lf_level[0]; P.lf_search_g[1] = P.lf_level_inter[0];
    for (int i = 0; i < 2; i++) { P.lf_level[i] = av1mi_lf_pool(P.lf_search_g[0], 7, 0); P.lf_level_inter[i] = av1mi_lf_pool(P.lf_search_g[1], 7, 0); }
  }
  P.enable_lr = (int)p.enable_lr;
  P.lr_chroma = r.lr_chroma;
  P.lr_unit_shift = r.lr_unit_shift;
  P.lr_lambda = r.lr_lambda;
  for (int rf = 0; rf < 4; rf++)
    for (int k = 0; k < 3; k++) {
      const BitString b = lr_code_of(rf, k); P.lr_code_len[rf][k] = b.len; P.lr_code_bits[rf][k] = b.bits;
      const BitString g = sgr_code_of(rf, k); P.sgr_code_len[rf][k] = g.len; P.sgr_code_bits[rf][k] = g.bits;
      const BitString u = lr_code_of_uv(rf, k); P.lr_code_len_uv[rf][k] = u.len; P.lr_code_bits_uv[rf][k] = u.bits;
    }
  return P;
}

// The block of parameters the reconstruction reads from device memory.  With adaptive quantisation P is followed by one copy per
// quantiser slot (av1mi_aq_slot) that differs in the quantiser steps, their reciprocals and the quantiser-matrix slice alone: the
// walk takes its superblock's copy, and everything else it reads there is what the first block holds.
std::vector<Av1miDevParams> slot_params(const Av1miDevParams &P) {
  const bool wide = P.frame_q != nullptr;   // the frame term: 28 blocks
  const int n_par = P.aq_map ? av1mi_aq_slots(wide) : 1;
  std::vector<Av1miDevParams> par((size_t)n_par, P);
  for (int sl = 1; sl < n_par; sl++) {
    Av1miDevParams &Q = par[(size_t)sl];
    set_quant_steps(Q, quant_steps(av1mi_aq_slot_qindex(sl, P.base_q_idx, wide), P.bit_depth));
    if (P.qm_tab) Q.qm_tab = P.qm_tab + (size_t)sl * 2 * AV1MI_QM_PLANE;
  }
  return par;
}

// dequantiser step per coefficient position (§7.12.3) and its reciprocal, for the square transform sizes 4..32
// with adaptive quantisation one slice per quantiser slot (av1mi_aq_slot): the superblock's steps through the frame's matrix
std::vector<Av1miQmEntry> make_qm_table(const Resolved &r) {
  static const int off[4] = { AV1MI_QM_4X4, AV1MI_QM_8X8, AV1MI_QM_16X16, AV1MI_QM_32X32 };
  const int slices = quant_slots(r);
  std::vector<Av1miQmEntry> tab((size_t)slices * 2 * AV1MI_QM_PLANE);
  for (int sl = 0; sl < slices; sl++) {
    const QuantSteps qs = quant_steps(av1mi_aq_slot_qindex(sl, r.qidx, r.fq != 0), (int)r.p.bit_depth);
    for (int pt = 0; pt < 2; pt++)
      for (int l2 = 2; l2 <= 5; l2++)
        for (int i = 0; i < (1 << (2 * l2)); i++) {
          const uint32_t q = (uint32_t)(i ? qs.ac_q : qs.dc_q);
          const uint32_t q2 = (q * av1_qm_iwt[r.qm_level][pt][off[l2 - 2] + i] + 16) >> 5;
          tab[(size_t)(sl * 2 + pt) * AV1MI_QM_PLANE + off[l2 - 2] + i] = { q2, recip32(q2) };
        }
  }
  return tab;
}

// Scene-cut rule (include/av1mi.h: av1mi_scene_cuts).  Integer only: d = mean absolute luma difference at 8-bit
// scale in Q8.  Mirrored by oracle/scenecut.py.
int scene_rule_step(av1mi_scene_state *st, int has_prev, uint64_t sad, uint64_t luma_samples, int bit_depth, uint32_t min_len) {
  if (!has_prev) { st->hist_n = 0; st->frames_since_cut = 1; return 1; }
  const uint64_t d = ((sad >> (bit_depth - 8)) << 8) / luma_samples;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < st->hist_n; i++) sum += st->hist_q8[i];
  const bool strong = st->hist_n ? (2 * d * st->hist_n >= 5 * sum && d >= 8 * 256) : d >= 24 * 256;
  if (strong && st->frames_since_cut >= min_len) { st->hist_n = 0; st->frames_since_cut = 1; return 1; }
  if (!strong) {  // in-scene sample: keep the last 8
    if (st->hist_n == 8) { for (int i = 0; i < 7; i++) st->hist_q8[i] = st->hist_q8[i + 1]; st->hist_n = 7; }
    st->hist_q8[st->hist_n++] = (uint32_t)d;
  }
  st->frames_since_cut++;
  return 0;
}

}  // namespace av1mi

using namespace av1mi;

extern "C" {

uint32_t av1mi_abi_version(void) { return AV1MI_ABI_VERSION; }
uint32_t av1mi_struct_sizes(uint32_t *sizes, uint32_t cap) {
  const uint32_t v[AV1MI_LAYOUT_ENTRIES] = {
    (uint32_t)sizeof(av1mi_params), (uint32_t)sizeof(av1mi_job), (uint32_t)sizeof(av1mi_report), (uint32_t)sizeof(av1mi_buf),
    (uint32_t)sizeof(av1mi_clip_info), (uint32_t)sizeof(av1mi_scene_state), (uint32_t)sizeof(av1mi_exec_job), (uint32_t)sizeof(av1mi_job_metrics),
    (uint32_t)offsetof(av1mi_job, params), (uint32_t)offsetof(av1mi_report, ms_h2d), (uint32_t)offsetof(av1mi_exec_job, params),
    (uint32_t)offsetof(av1mi_job_metrics, frames_encoded) };
  for (uint32_t i = 0; i < AV1MI_LAYOUT_ENTRIES && i < cap && sizes; i++) sizes[i] = v[i];
  return AV1MI_LAYOUT_ENTRIES;
}
uint32_t av1mi_cq_to_qindex(uint32_t cq) { return kQuantizerToQindex[cq > 63 ? 63 : cq]; }

void av1mi_default_params(av1mi_params *p, uint32_t w, uint32_t h, uint32_t bd) {
  memset(p, 0, sizeof(*p));
  p->width = w; p->height = h; p->bit_depth = bd;
  p->cq_level = 30; p->keyint = 1; p->block_log2 = 5; p->cdf_update = 1; p->enable_cdef = 1;
  p->cdef_y_pri = 2; p->cdef_y_sec = 0; p->cdef_uv_pri = 1; p->cdef_uv_sec = 0; p->cdef_damping = 5;
  p->qm_min = 8; p->qm_max = 15;  // used when enable_qm = 1
}

int av1mi_write_headers(const av1mi_params *p, uint8_t *seq_hdr, size_t *seq_len, uint8_t *frame_hdr, size_t *frame_hdr_bits) {
  Resolved r;
  int rc = resolve(p, &r);
  if (rc) return rc;
  std::vector<uint8_t> s = make_sequence_header(r);
  size_t bits = 0;
  std::vector<uint8_t> f = make_frame_header(r, &bits);
  if (seq_hdr && seq_len) { if (*seq_len < s.size()) return AV1MI_E_INVALID_ARG; memcpy(seq_hdr, s.data(), s.size()); }
  if (seq_len) *seq_len = s.size();
  if (frame_hdr) memcpy(frame_hdr, f.data(), f.size());
  if (frame_hdr_bits) *frame_hdr_bits = bits;
  return AV1MI_OK;
}
}  // extern "C"
