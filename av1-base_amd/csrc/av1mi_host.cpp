// av1mi_host.cpp - host side of libav1mi behind the C ABI of include/av1mi.h.
//
// Mirrors the reference's encode boundary: `run_av1an(&Av1anEncodeParams) -> Result<(), EncodeError>`
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139) becomes av1mi_encode_file(); the
// per-chunk work av1an farms out to SVT-AV1 workers (`--workers`, av1an.rs:100-101) becomes
// av1mi_encode_chunk() on one context (= one GPU + one HIP stream).  No CPU encode path exists
// here: without a HIP device every entry point fails with AV1MI_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/av1mi.h"
#include "av1_tables.h"
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "lr_fit_rule.h"
#include "lr_rate_rule.h"
#include "wiener_fit_rule.h"
#include "deblock_pieces.h"
#include "aq_rule.h"
#include "part_inter_rule.h"
#include "tf_rule.h"

namespace {

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

int tile_log2(int blk, int target) { int k = 0; while ((blk << k) < target) k++; return k; }
int bits_for(unsigned v) { int n = 0; while (v) { n++; v >>= 1; } return n ? n : 1; }

// quantiser steps of a quantiser index, and their reciprocals ceil(2^32 / q)
struct QuantSteps { int dc_q, ac_q; uint32_t dc_recip, ac_recip; };
uint32_t recip32(uint32_t q) { return (uint32_t)((((uint64_t)1 << 32) + q - 1) / q); }
QuantSteps quant_steps(int qindex, int bit_depth) {
  const int dc = bit_depth == 8 ? av1_dc_q8[qindex] : av1_dc_q10[qindex], ac = bit_depth == 8 ? av1_ac_q8[qindex] : av1_ac_q10[qindex];
  return { dc, ac, recip32((uint32_t)dc), recip32((uint32_t)ac) };
}
void set_quant_steps(Av1miDevParams &P, const QuantSteps &q) { P.dc_q = q.dc_q; P.ac_q = q.ac_q; P.dc_recip = q.dc_recip; P.ac_recip = q.ac_recip; }
// coefficient q context: which of the four sets of default coefficient CDFs the frames start from
int q_context(int qidx) { return qidx <= 20 ? 0 : (qidx <= 60 ? 1 : (qidx <= 120 ? 2 : 3)); }

struct Resolved {
  av1mi_params p;
  int qidx;
  QuantSteps q;                       // quantiser steps of qidx at p.bit_depth
  int cw, ch;                         // coded size: p.width / p.height rounded up to multiples of 8
  bool padded;                        // the coded size is not the signalled one: frames are edge-extended in and cropped out
  int sb_cols, sb_rows;
  int tile_sb, tile_cols, tile_rows;  // tiles of tile_sb x tile_sb superblocks (1, or 2 beyond 64 superblocks either way)
  int qm_level;                       // quantiser-matrix level of all planes (15 = flat); only meaningful with p.enable_qm
  int lr_chroma;                      // enable_lr 3 / 4: U and V restored as well (p.enable_lr then holds the type: 1 / 2)
  int aq;                             // strength of the adaptive quantisation, 0 = off (p.cq_level then holds the CQ level alone)
  uint32_t lr_fit_mask;               // enable_lr bit 8: the parameter sets the self-guided fit searches, 0 = no fit (p.enable_lr holds the type)
  int lr_wfit;                        // enable_lr bit 10: the Wiener fit (p.enable_lr holds the type)
  int lr_unit_shift;                  // enable_lr bits 12-13: luma restoration units of 64 << lr_unit_shift samples (0 .. 2)
  uint32_t lr_lambda;                 // enable_lr bits 14 and 15: the rate term's lambda (lr_rate_rule.h), 0 = the decisions go by the error alone
  int tf_frames, tf_strength;         // me_presearch bits 8-10 and 12-14: the key frames' temporal filter (tf_rule.h), 0 followers = off (p.me_presearch then holds bit 0 alone)
};

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
  // ... and bits 8-10 of the field are the strength of the adaptive quantisation, 0 .. 4; nothing above them
  r->aq = (int)AV1MI_AQ_STRENGTH(p.cq_level);
  if ((p.cq_level >> 11) || r->aq > AV1MI_AQ_MAX_STRENGTH) return AV1MI_E_INVALID_ARG;
  p.cq_level = AV1MI_CQ_LEVEL(p.cq_level);
  if (p.cq_level == 0 || p.cq_level > 63 || p.film_grain > 50) return AV1MI_E_INVALID_ARG;
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
int deblock_level(const Resolved &r, bool key) {
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
std::vector<uint8_t> make_frame_header(const Resolved &r, size_t *hdr_bits, uint32_t frame_number = 0, bool inter = false, size_t *cdef_str_bit = nullptr,
                                       size_t *lf_bit = nullptr) {
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
  b.put((uint32_t)r.qidx, 8);
  b.put(0, 1);  // DeltaQYDc
  b.put(0, 1);  // DeltaQUDc
  b.put(0, 1);  // DeltaQUAc
  b.put(r.p.enable_qm ? 1 : 0, 1);  // using_qmatrix
  if (r.p.enable_qm) { b.put((uint32_t)r.qm_level, 4); b.put((uint32_t)r.qm_level, 4); }  // qm_y, qm_u (= qm_v: separate_uv_delta_q = 0)
  b.put(0, 1);  // segmentation_enabled
  if (r.qidx > 0) b.put(r.aq ? 1 : 0, 1);  // delta_q_present
  if (r.aq) {
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
    b.put(2, 4); b.put(0, 8); b.put(sy, 8); b.put(255, 8); b.put(sy, 8);  // num_y_points + points
    b.put(0, 1);                                              // chroma_scaling_from_luma
    for (int pl = 0; pl < 2; pl++) { b.put(2, 4); b.put(0, 8); b.put(sc, 8); b.put(255, 8); b.put(sc, 8); }
    b.put(3, 2);                                              // grain_scaling_minus_8
    b.put(0, 2);                                              // ar_coeff_lag
    b.put(128, 8); b.put(128, 8);                             // ar_coeffs_cb/cr_plus_128[0]
    b.put(0, 2);                                              // ar_coeff_shift_minus_6
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
BitString sgr_code_of(int ref, int cand) {
  static const int mid[2] = { -32, 31 };
  return av1mi_lr_sgr_code(av1mi_sgr_cand[cand][0], av1mi_sgr_cand[cand][1], av1mi_sgr_cand[cand][2], ref ? av1mi_sgr_cand[ref - 1][1] : mid[0], ref ? av1mi_sgr_cand[ref - 1][2] : mid[1]);
}
// ref: 0 = Wiener_Taps_Mid (tile start), r = candidate r-1 (the previous unit of the tile that was coded with a filter)
BitString lr_code_of(int ref, int cand) {
  static const int tmin[3] = { -5, -23, -17 }, tmax[3] = { 10, 8, 46 }, tk[3] = { 1, 2, 3 }, mid[3] = { 3, -7, 15 };
  BitString b;
  for (int pass = 0; pass < 2; pass++)
    for (int j = 0; j < 3; j++) lr_put_signed_ref(b, tmin[j], tmax[j] + 1, tk[j], ref ? av1mi_wiener_cand[ref - 1][j] : mid[j], av1mi_wiener_cand[cand][j]);
  return b;
}
// the same for a chroma unit: taps 1 and 2 of each pass, against the plane's RefLrWiener
BitString lr_code_of_uv(int ref, int cand) {
  static const int tmin[3] = { -5, -23, -17 }, tmax[3] = { 10, 8, 46 }, tk[3] = { 1, 2, 3 }, mid[3] = { 3, -7, 15 };
  BitString b;
  for (int pass = 0; pass < 2; pass++)
    for (int j = 1; j < 3; j++) lr_put_signed_ref(b, tmin[j], tmax[j] + 1, tk[j], ref ? av1mi_wiener_cand_uv[ref - 1][j] : mid[j], av1mi_wiener_cand_uv[cand][j]);
  return b;
}

// default CDF blob for one q context in the layout of Av1miCdfLayout (inverted, 0, counter)
template <size_t W>
void emit_rows(std::vector<uint16_t> &v, size_t off, const uint16_t (*rows)[W], int nrows, int row_stride, const int *nsym, int nsym_const) {
  for (int i = 0; i < nrows; i++) {
    int n = nsym ? nsym[i] : nsym_const;
    for (int k = 0; k < n - 1; k++) v[off + (size_t)i * row_stride + k] = (uint16_t)(32768 - rows[i][k]);
  }
}
std::vector<uint16_t> make_cdf_blob(int qidx) {
  typedef Av1miCdfLayout CL;
  const int q = q_context(qidx);
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

// ------------------------------------------------------------------ context
// Points of one chunk on the context's streams; the report's stage times are the intervals between them.  Main stream: start, source
// on the device, reconstruction (and the rest of the kind's work before entropy coding), symbolize, entropy coding (groups joined), packing
// and download done.  Second stream: its work beside the range coder.  Third: an inter chunk's groups.  Fourth: the edge tiles' fork, join.
enum ChunkEvent { EV_START, EV_SRC_READY, EV_RECON_DONE, EV_SYM_DONE, EV_ENTROPY_DONE, EV_PACK_DONE, EV_DOWNLOAD_DONE,
                  EV_CDEF_START, EV_CDEF_DONE, EV_GROUPS_JOINED, EV_EDGE_FORK, EV_EDGE_JOIN, EV_COUNT };

// A context's device workspace and host staging buffer.  Every buffer comes from ws_alloc, which records it; free_workspace frees
// what was recorded and resets all of it to these defaults.
struct Workspace {
  size_t cap_frames = 0;
  int scale = 0;       // the capacity multiplier the workspace was allocated with
  Resolved res = {};   // ... and the parameters of its last chunk
  void *d_src = nullptr, *d_rec = nullptr, *d_fin = nullptr;
  int16_t *d_levels = nullptr; Av1miBlkInfo *d_blk = nullptr;
  uint8_t *d_slots = nullptr, *d_out = nullptr, *d_hdr = nullptr;
  uint16_t *d_cdf = nullptr;
  Av1miDevParams *d_params = nullptr;  // copy of P for the kernels that read their parameters through a pointer (recon)
  uint32_t *d_tile_bytes = nullptr, *d_tile_off = nullptr, *d_frame_size = nullptr, *d_payload = nullptr, *d_sym = nullptr;
  uint32_t *d_streams = nullptr, *d_combos = nullptr;
  unsigned long long *d_sse = nullptr;
  // symbolize's tile order (tile_weight_rule.h): the classes' counters - the head of the block d_sse lies in, so that one fill clears
  // both - and the rows [AV1MI_TILE_CLASSES][cap_frames x tiles] the reconstruction fills
  uint32_t *d_sym_count = nullptr, *d_sym_order = nullptr;
  Av1miChunkRecord *d_record = nullptr;   // symbol counts, overflow flag, then frame_off[cap_frames + 1] (av1mi_launch_pack)
  unsigned long long *d_me = nullptr;  // motion search results per 8x8 unit per frame
  void *d_stage = nullptr;             // sizes that are not multiples of 8: frames in the caller's tight layout (input / reconstruction out)
  void *d_cd = nullptr;                // loop restoration on: CDEF output (d_fin then holds the restored frames)
  unsigned long long *d_me_sub = nullptr;  // sub-sample refinement: refined [frame][8x8 unit] keys (me_kernel.hip)
  uint16_t *d_quarter = nullptr;           // me_presearch: quarter-resolution luma of every frame of the chunk
  uint32_t *d_centre = nullptr;            // me_presearch: centre code of the full search per [frame][superblock]
  uint32_t *d_part = nullptr;              // content-driven partition: split mask per [frame][superblock] (partition_kernel)
  uint32_t *d_me64 = nullptr;              // 64x64 leaves: the search's [frame][superblock][candidate] SAD table
  uint32_t *d_nodes = nullptr;             // partition_search = 2: the node-mode search's [frame][level][node] keys (part_inter_rule.h)
  uint16_t *d_aq_act = nullptr;            // adaptive quantisation: E per [frame][superblock] (aq_activity_kernel)
  uint8_t *d_aq_map = nullptr;             // ... the quantiser index per [frame][superblock] (aq_map_kernel)
  uint32_t *d_tf_mv = nullptr;             // temporal filter: the search's keys per [key frame][follower][16x16 block] (tf_kernel.hip)
  Av1miQmEntry *d_qm = nullptr;        // quantiser-matrix steps (Av1miDevParams::qm_tab), one slice per quantiser slot, valid for qm_key = (slices, level, qidx, bit depth)
  std::vector<Av1miQmEntry> h_qm; int qm_key = -1;
  uint8_t *d_lrc = nullptr;            // per restoration unit: 0 = off, k = candidate k-1
  unsigned long long *d_lrsse = nullptr;  // per restoration unit: the candidates' SSE sums (scratch of lr_kernel.hip's two phases)
  // the self-guided fit: one block, laid out for the chunk's units (ensure_workspace) - errors and records, which the host fetches
  // into h_fit with one copy, then sums and codes - so that one fill clears a chunk's part
  Av1miLrFit fit = {};
  uint8_t *d_fit = nullptr, *h_fit = nullptr;
  // the Wiener fit, likewise: errors and records at the head (h_wfit), then sums and codes
  Av1miLrWfit wfit = {};
  uint8_t *d_wfit = nullptr, *h_wfit = nullptr;
  unsigned long long *d_cdef_err = nullptr;  // CDEF strength search: per [frame][superblock] the 24 candidates' squared errors
  int8_t *d_cdef_idx = nullptr;              // ... per [frame][superblock] the index into the frame's set (-1: not coded)
  uint8_t *d_cdef_sel = nullptr;             // ... per frame the set: 8 slots of pair indices
  unsigned long long *d_lf_err = nullptr;    // deblocking level search: per [frame][plane] the 16 candidates' squared errors, and behind
  uint8_t *d_lf_sel = nullptr;               // them, in the same block, per frame the four levels; h_lf: where one copy lands both
  uint8_t *h_lf = nullptr;
  uint8_t *h_out = nullptr;            // host staging (pinned), for when the caller's buffer cannot be page-locked
  // Page-locked host side of the small transfers.  The chunk constants - header blob, default CDFs, parameters - are the same for
  // every chunk of a job: h_hdr / h_cdf / h_params hold what d_hdr / d_cdf / d_params hold, and prepare_chunk uploads only what differs.
  uint8_t *h_hdr = nullptr; uint16_t *h_cdf = nullptr; Av1miDevParams *h_params = nullptr;
  size_t hdr_bytes = 0;                // bytes of h_hdr that d_hdr is known to hold; 0: unknown (the strength search writes into d_hdr)
  int cdf_qidx = -1;                   // the quantiser index d_cdf was made for (the blob depends on nothing else); -1: none
  int cdf_bs_log2 = -1;                // ... and the leaf size its compact image behind the blob was made for
  int params_on_device = 0;            // d_params holds the first so many blocks of h_params (1, or AV1MI_AQ_SLOTS with adaptive quantisation)
  Av1miChunkRecord *h_record = nullptr; unsigned long long *h_sse = nullptr;   // d_record and d_sse land here
  size_t out_cap = 0, me64_bytes = 0, nodes_bytes = 0, h_out_cap = 0, tf_mv_bytes = 0;   // bytes of d_out, d_me64, d_nodes, h_out, d_tf_mv
  std::vector<std::pair<void *, bool>> owned;   // every buffer above: (address, page-locked host memory)
};

// (Re)allocates one buffer of the workspace - device memory, or page-locked host memory with `host` - and records it for free_workspace
template <class T>
hipError_t ws_alloc(Workspace &w, T *&p, size_t bytes, bool host = false) {
  for (auto b = w.owned.begin(); p && b != w.owned.end(); ++b)   // a buffer that grows: the old one goes
    if (b->first == (void *)p) { (void)(b->second ? hipHostFree(p) : hipFree(p)); w.owned.erase(b); break; }
  void *v = nullptr;
  const hipError_t e = host ? hipHostMalloc(&v, bytes, hipHostMallocDefault) : hipMalloc(&v, bytes);
  if (e == hipSuccess) w.owned.emplace_back(v, host);
  p = (T *)v;
  return e;
}

}  // namespace

struct av1mi_ctx {
  int device = -1;
  hipStream_t stream = nullptr;   // the four streams come from and go back to a process-wide pool (av1mi_ctx_create)
  hipStream_t stream2 = nullptr;  // CDEF + SSE run here, beside the entropy kernels on `stream`
  hipStream_t stream3 = nullptr;  // inter chunks: entropy coding of finished groups of frames, beside the frame-by-frame chain
  hipStream_t stream4 = nullptr;  // the frame-edge tiles' symbolize variant, beside the regular one on `stream` (av1mi_launch_entropy)
  hipEvent_t ev[EV_COUNT] = {};
  std::vector<hipEvent_t> me_ev;       // per frame: its motion search has finished (second stream -> main stream)
  std::vector<hipEvent_t> grp_ev;      // per group of frames of an inter chunk: reconstructed (main stream -> third stream)
  std::string err;
  int cap_scale = 1;   // per-tile symbol-stream / bitstream-slot capacity multiplier (1, 2, 4, ... 64)
  Workspace ws;
  Av1miDevParams P = {};
  // the last encoded chunk's deblocking levels (4 per frame) and level-search errors (48 per frame; zeros without the search):
  // av1mi_lf_search_result.  Empty: no chunk, or the last one failed
  std::vector<uint8_t> lf_levels;
  std::vector<unsigned long long> lf_errs;
  // ... and its self-guided fit (av1mi_lr_fit_result): the units of its frames over three planes, and whether the fit ran - the errors
  // and records are then the head of ws.h_fit
  size_t fit_units = 0;
  uint32_t fit_plane_units = 0;   // the units of one plane of one frame (av1mi_lr_fit_units)
  bool fit_on = false;
  bool wfit_on = false;           // ... and its Wiener fit (av1mi_lr_wiener_fit_result): the head of ws.h_wfit
  bool sym_order = true;          // AV1MI_SYM_ORDER, read when the context is made: 0 = symbolize in natural tile order everywhere
  uint32_t sym_tiles = 0;         // the tiles of the last chunk's weight-ordered table (av1mi_sym_order_result); 0: natural order
  bool part_inter = false;        // this chunk's inter frames are partitioned from the search's node costs (partition_search = 2)
  bool pi_keys = false;           // ... and it was coded in that mode: its search keys are reported too
  uint32_t pi_frames = 0, pi_units = 0, pi_sbs = 0;   // the last chunk with a partition map: frames, 8x8 units and superblocks per frame (av1mi_inter_partition_result)
};

namespace {

void set_err(av1mi_ctx *c, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
}

#define HIPCHK(c, call)                                                                          \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      set_err((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__);   \
      return e__ == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP;                             \
    }                                                                                            \
  } while (0)

void free_workspace(av1mi_ctx *c) {
  for (auto &b : c->ws.owned) (void)(b.second ? hipHostFree(b.first) : hipFree(b.first));
  c->ws = Workspace();
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
// whether the filter changes any frame of the chunk: some key frame has a follower (its first key frame then has)
bool tf_runs(const Resolved &r, size_t n_frames) { return av1mi_tf_followers(r.tf_frames, (int)r.p.keyint, (int)n_frames, 0) > 0; }

int ensure_workspace(av1mi_ctx *c, const Resolved &r, uint32_t n_frames) {
  const av1mi_params &p = r.p;
  Workspace &w = c->ws;
  // the per-tile buffers (symbol streams, bitstream slots, packed output) are sized by the tile grid and the per-tile
  // capacities, which follow tile_sb: a context that switches tile_sb at the same frame size must not reuse them
  // (648x360: 66 tiles x 4096 entries at tile_sb 1, but 18 x 16384 at tile_sb 2)
  const bool same = w.cap_frames >= n_frames && w.res.p.width == p.width && w.res.p.height == p.height && w.res.p.bit_depth == p.bit_depth &&
                    w.scale == c->cap_scale && w.res.tile_sb == r.tile_sb;
  const int bps = p.bit_depth > 8 ? 2 : 1;
  const size_t frame_bytes = (size_t)r.cw * r.ch * 3 / 2 * bps;   // coded size
  const size_t nsb = (size_t)r.sb_cols * r.sb_rows, ntile = (size_t)r.tile_cols * r.tile_rows, nb8 = (size_t)(r.cw / 8) * (r.ch / 8);
  if (!same) {
    free_workspace(c);
    const size_t nf = n_frames, slot = (size_t)tile_slot_bytes(r, c->cap_scale);
    for (void **b : { &w.d_src, &w.d_rec, &w.d_fin }) HIPCHK(c, ws_alloc(w, *b, nf * frame_bytes));
    HIPCHK(c, ws_alloc(w, w.d_levels, nf * nsb * AV1MI_SB_LEVELS * sizeof(int16_t)));
    HIPCHK(c, ws_alloc(w, w.d_blk, nf * nb8 * sizeof(Av1miBlkInfo)));
    // on the context's own stream: hipMemset would run on the null stream, which a non-blocking stream does not wait
    // for - the fill could land after the first reconstruction kernel had written its block info
    HIPCHK(c, hipMemsetAsync(w.d_blk, 0, nf * nb8 * sizeof(Av1miBlkInfo), c->stream));
    HIPCHK(c, ws_alloc(w, w.d_slots, nf * ntile * slot * 2));  // 16-bit pre-carry entries, one per output byte
    w.out_cap = nf * (ntile * (slot + 4) + 256);
    HIPCHK(c, ws_alloc(w, w.d_out, w.out_cap));
    HIPCHK(c, ws_alloc(w, w.d_hdr, 256 + nf * 512));
    HIPCHK(c, ws_alloc(w, w.d_cdf, Av1miCdfCompact::BLOB_WORDS * sizeof(uint16_t)));   // the blob and its compact image
    HIPCHK(c, ws_alloc(w, w.d_params, AV1MI_AQ_SLOTS * sizeof(Av1miDevParams)));
    for (uint32_t **b : { &w.d_tile_bytes, &w.d_tile_off, &w.d_sym, &w.d_combos }) HIPCHK(c, ws_alloc(w, *b, nf * nsb * 4));
    HIPCHK(c, ws_alloc(w, w.d_streams, nf * ntile * (size_t)tile_stream_cap(r, c->cap_scale) * 4));
    for (uint32_t **b : { &w.d_frame_size, &w.d_payload }) HIPCHK(c, ws_alloc(w, *b, nf * 4));
    HIPCHK(c, ws_alloc(w, w.d_record, sizeof(Av1miChunkRecord) + (nf + 1) * 8));
    HIPCHK(c, ws_alloc(w, w.d_sym_count, AV1MI_TILE_CLASSES * 4 + nf * 3 * 8));
    w.d_sse = reinterpret_cast<unsigned long long *>(w.d_sym_count + AV1MI_TILE_CLASSES);
    HIPCHK(c, ws_alloc(w, w.d_sym_order, (size_t)AV1MI_TILE_CLASSES * nf * ntile * 4));
    {  // the five small host mirrors share one page-locked block: an allocation of page-locked memory costs far more than they hold
      auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
      const size_t b_hdr = up(256 + nf * 512), b_cdf = up(Av1miCdfCompact::BLOB_WORDS * sizeof(uint16_t)), b_par = up(AV1MI_AQ_SLOTS * sizeof(Av1miDevParams)),
                   b_rec = up(sizeof(Av1miChunkRecord) + (nf + 1) * 8), b_sse = up(nf * 3 * 8);
      uint8_t *h = nullptr;
      HIPCHK(c, ws_alloc(w, h, b_hdr + b_cdf + b_par + b_rec + b_sse, true));
      w.h_hdr = h; h += b_hdr;
      w.h_cdf = reinterpret_cast<uint16_t *>(h); h += b_cdf;
      w.h_params = reinterpret_cast<Av1miDevParams *>(h); h += b_par;
      w.h_record = reinterpret_cast<Av1miChunkRecord *>(h); h += b_rec;
      w.h_sse = reinterpret_cast<unsigned long long *>(h);
    }
    HIPCHK(c, ws_alloc(w, w.d_me, nf * nb8 * 8));
    w.cap_frames = n_frames; w.scale = c->cap_scale;
  }
  const size_t nf = w.cap_frames;
  if (r.padded && !w.d_stage) HIPCHK(c, ws_alloc(w, w.d_stage, caller_bytes(r, nf)));
  if (p.partition_search && !w.d_part) HIPCHK(c, ws_alloc(w, w.d_part, nf * nsb * sizeof(uint32_t)));
  if (p.me_presearch && !w.d_quarter) {
    HIPCHK(c, ws_alloc(w, w.d_quarter, nf * (size_t)(r.cw / 4) * (r.ch / 4) * sizeof(uint16_t)));
    HIPCHK(c, ws_alloc(w, w.d_centre, nf * nsb * sizeof(uint32_t)));
  }
  if (p.subpel && !w.d_me_sub) HIPCHK(c, ws_alloc(w, w.d_me_sub, nf * nb8 * 8));  // output of the sub-sample refinement
  if (p.block_log2 >= 6 && p.keyint > 1) {   // candidate table of the 64x64 leaves' motion search
    const size_t nc = 2 * (size_t)(p.me_range ? p.me_range : 8) + 1, need = nf * nsb * nc * nc * sizeof(uint32_t);
    if (w.me64_bytes < need) { w.me64_bytes = 0; HIPCHK(c, ws_alloc(w, w.d_me64, need)); w.me64_bytes = need; }
  }
  if (p.partition_search == 2 && p.keyint > 1) {   // node tables of the inter frames' partition decision, on first use
    const size_t need = nf * av1mi_pi_frame_nodes(r.ch / 8, r.cw / 8) * sizeof(uint32_t);
    if (w.nodes_bytes < need) { w.nodes_bytes = 0; HIPCHK(c, ws_alloc(w, w.d_nodes, need)); w.nodes_bytes = need; }
  }
  if (r.tf_frames) {   // the temporal filter's keys, on first use (and when a chunk has more key frames or followers than any before)
    const size_t need = tf_mv_entries(r, n_frames) * sizeof(uint32_t);
    if (w.tf_mv_bytes < need) { w.tf_mv_bytes = 0; HIPCHK(c, ws_alloc(w, w.d_tf_mv, need)); w.tf_mv_bytes = need; }
  }
  if (r.aq && !w.d_aq_map) {
    HIPCHK(c, ws_alloc(w, w.d_aq_act, nf * nsb * sizeof(uint16_t)));
    HIPCHK(c, ws_alloc(w, w.d_aq_map, nf * nsb));
  }
  if (p.cdef_search && (!w.d_cdef_err || !w.d_cdef_idx || !w.d_cdef_sel)) {
    HIPCHK(c, ws_alloc(w, w.d_cdef_err, nf * nsb * 24 * sizeof(unsigned long long)));
    HIPCHK(c, ws_alloc(w, w.d_cdef_idx, nf * nsb));
    HIPCHK(c, ws_alloc(w, w.d_cdef_sel, nf * 8));
  }
  if (p.deblock == 2 && (!w.d_lf_err || !w.h_lf)) {   // (both: the second allocation may have failed on an earlier chunk)
    HIPCHK(c, ws_alloc(w, w.d_lf_err, nf * (3 * AV1MI_LF_CANDS * sizeof(unsigned long long) + 4)));
    w.d_lf_sel = reinterpret_cast<uint8_t *>(w.d_lf_err + nf * 3 * AV1MI_LF_CANDS);
    HIPCHK(c, ws_alloc(w, w.h_lf, nf * (3 * AV1MI_LF_CANDS * sizeof(unsigned long long) + 4), true));
  }
  if (p.enable_lr && !w.d_cd) {   // unit choices and sums for three planes (enable_lr 3 / 4) of 64x64 units, whichever value and unit size
                                  // this chunk has: the buffers stay with the geometry while enable_lr changes
    HIPCHK(c, ws_alloc(w, w.d_cd, nf * frame_bytes));
    HIPCHK(c, ws_alloc(w, w.d_lrc, 3 * nf * nsb + 64));
    HIPCHK(c, ws_alloc(w, w.d_lrsse, (3 * nf * nsb + 64) * 8 * sizeof(unsigned long long)));
  }
  if (r.lr_fit_mask && (!w.d_fit || !w.h_fit)) {   // for three planes, like the unit sums: the buffers stay while enable_lr changes
    const size_t units = 3 * nf * nsb + 64;
    HIPCHK(c, ws_alloc(w, w.d_fit, av1mi_lr_fit_bytes(units)));
    HIPCHK(c, ws_alloc(w, w.h_fit, av1mi_lr_fit_result_bytes(units), true));
  }
  if (r.lr_fit_mask) w.fit = av1mi_lr_fit_split(w.d_fit, fit_chunk_units(r, n_frames), r.lr_fit_mask);   // this chunk's units, from the head of the block
  w.fit.mask = r.lr_fit_mask;
  if (r.lr_wfit && (!w.d_wfit || !w.h_wfit)) {
    const size_t units = 3 * nf * nsb + 64;
    HIPCHK(c, ws_alloc(w, w.d_wfit, av1mi_lr_wfit_bytes(units)));
    HIPCHK(c, ws_alloc(w, w.h_wfit, av1mi_lr_wfit_result_bytes(units), true));
  }
  if (r.lr_wfit) w.wfit = av1mi_lr_wfit_split(w.d_wfit, fit_chunk_units(r, n_frames));
  w.res = r;
  if (p.enable_qm && r.qm_level < 15) {
    // dequantiser step per coefficient position (§7.12.3) and its reciprocal, for the square transform sizes 4..32
    // with adaptive quantisation one slice per quantiser slot (av1mi_aq_slot): the superblock's steps through the frame's matrix
    if (!w.d_qm) HIPCHK(c, ws_alloc(w, w.d_qm, AV1MI_AQ_SLOTS * 2 * AV1MI_QM_PLANE * sizeof(Av1miQmEntry)));
    const int slices = r.aq ? AV1MI_AQ_SLOTS : 1;
    const int key = (slices << 24) | (r.qm_level << 16) | (r.qidx << 4) | (int)p.bit_depth;
    if (w.qm_key != key) {
      static const int off[4] = { AV1MI_QM_4X4, AV1MI_QM_8X8, AV1MI_QM_16X16, AV1MI_QM_32X32 };
      w.h_qm.resize((size_t)slices * 2 * AV1MI_QM_PLANE);
      for (int sl = 0; sl < slices; sl++) {
        const QuantSteps qs = quant_steps(av1mi_aq_slot_qindex(sl, r.qidx), (int)p.bit_depth);
        for (int pt = 0; pt < 2; pt++)
          for (int l2 = 2; l2 <= 5; l2++)
            for (int i = 0; i < (1 << (2 * l2)); i++) {
              const uint32_t q = (uint32_t)(i ? qs.ac_q : qs.dc_q);
              const uint32_t q2 = (q * av1_qm_iwt[r.qm_level][pt][off[l2 - 2] + i] + 16) >> 5;
              w.h_qm[(size_t)(sl * 2 + pt) * AV1MI_QM_PLANE + off[l2 - 2] + i] = { q2, recip32(q2) };
            }
      }
      HIPCHK(c, hipMemcpyAsync(w.d_qm, w.h_qm.data(), w.h_qm.size() * sizeof(Av1miQmEntry), hipMemcpyHostToDevice, c->stream));
      w.qm_key = key;
    }
  }
  return AV1MI_OK;
}

// The kernels' parameters of a chunk of `n_frames` frames: `r` at the coded size, the per-tile capacities of multiplier `scale` and the
// workspace buffers the kernels find through them.  The header sizes follow with the headers (prepare_chunk).
Av1miDevParams dev_params(const Resolved &r, uint32_t n_frames, int scale, const uint32_t *part, const Av1miQmEntry *qm, const uint8_t *aq_map,
                          unsigned long long *cdef_err, int8_t *cdef_idx, uint8_t *cdef_sel, unsigned long long *lf_err, uint8_t *lf_sel,
                          Av1miChunkRecord *record, const uint32_t *tile_symbols, const uint32_t *lr_fit_code, const uint32_t *lr_wfit_code) {
  const av1mi_params &p = r.p;
  Av1miDevParams P;
  memset(&P, 0, sizeof(P));
  P.width = r.cw; P.height = r.ch; P.bit_depth = p.bit_depth; P.true_w = (int)p.width; P.true_h = (int)p.height;
  P.mi_rows = r.ch / 4; P.mi_cols = r.cw / 4; P.b8_rows = r.ch / 8; P.b8_cols = r.cw / 8; P.sb_rows = r.sb_rows; P.sb_cols = r.sb_cols;
  P.tile_sb = r.tile_sb; P.tile_rows = r.tile_rows; P.tile_cols = r.tile_cols;
  P.n_frames = (int)n_frames;
  P.base_q_idx = r.qidx;
  P.qctx = q_context(r.qidx);
  set_quant_steps(P, r.q);
  P.using_qm = p.enable_qm ? 1 : 0; P.qm_y = P.qm_uv = r.qm_level;
  P.qm_tab = p.enable_qm && r.qm_level < 15 ? qm : nullptr;
  P.max_bs_log2 = (int)p.block_log2;
  P.min_bs_log2 = p.partition_search ? (int)p.min_block_log2 : (int)p.block_log2;
  P.part_map = p.partition_search ? part : nullptr;
  P.aq_map = r.aq ? aq_map : nullptr;
  P.mode_mask = p.intra_mode_mask ? (p.intra_mode_mask & 0x1FFF) : 0x0007;  // default candidates: DC, V, H
  P.angle_delta = p.intra_angle_delta ? 1 : 0; P.edge_filter = p.intra_edge_filter ? 1 : 0; P.cfl = p.cfl ? 1 : 0; P.tx_search = p.tx_search ? 1 : 0;
  P.enable_cdef = p.enable_cdef ? 1 : 0;
  P.cdef_y_pri = p.cdef_y_pri; P.cdef_y_sec = p.cdef_y_sec; P.cdef_uv_pri = p.cdef_uv_pri; P.cdef_uv_sec = p.cdef_uv_sec;
  P.cdef_damping = p.cdef_damping; P.cdef_search = (int)p.cdef_search;
  if (p.cdef_search) { P.cdef_bits = (int)p.cdef_search - 1; P.cdef_err = cdef_err; P.cdef_idx = cdef_idx; P.cdef_sel = cdef_sel; }
  P.disable_cdf_update = p.cdf_update ? 0 : 1;
  P.stride_y = r.cw; P.stride_c = r.cw / 2; P.frame_samples = (long)r.cw * r.ch * 3 / 2;
  P.plane_off_u = (long)r.cw * r.ch; P.plane_off_v = P.plane_off_u + (long)(r.cw / 2) * (r.ch / 2);
  P.tile_slot_bytes = tile_slot_bytes(r, scale); P.stream_cap = tile_stream_cap(r, scale); P.tile_size_bytes = 4;
  P.keyint = (int)p.keyint; P.me_range = (int)p.me_range; P.subpel = p.subpel ? 1 : 0; P.me_presearch = p.me_presearch ? 1 : 0;
  P.hdr_slot_bytes = 512;
  for (int i = 0; i < 4; i++) { P.lf_level[i] = deblock_level(r, true); P.lf_level_inter[i] = deblock_level(r, false); }
  if (p.deblock == 2) {   // the level search: the header's placeholders (luma at least 1: every frame is deblocked)
    P.lf_search = 1; P.lf_err = lf_err; P.lf_sel = lf_sel;
    P.lf_search_g[0] = P.lf_level[0]; P.lf_search_g[1] = P.lf_level_inter[0];
    for (int i = 0; i < 2; i++) { P.lf_level[i] = av1mi_lf_pool(P.lf_search_g[0], 7, 0); P.lf_level_inter[i] = av1mi_lf_pool(P.lf_search_g[1], 7, 0); }
  }
  P.enable_lr = (int)p.enable_lr;
  P.lr_chroma = r.lr_chroma;
  P.lr_unit_shift = r.lr_unit_shift;
  P.lr_lambda = r.lr_lambda;
  P.lr_fit_code = r.lr_fit_mask ? lr_fit_code : nullptr;
  P.lr_wfit_code = r.lr_wfit ? lr_wfit_code : nullptr;
  P.chunk_record = record; P.tile_symbols = tile_symbols;
  for (int rf = 0; rf < 4; rf++)
    for (int k = 0; k < 3; k++) {
      const BitString b = lr_code_of(rf, k); P.lr_code_len[rf][k] = b.len; P.lr_code_bits[rf][k] = b.bits;
      const BitString g = sgr_code_of(rf, k); P.sgr_code_len[rf][k] = g.len; P.sgr_code_bits[rf][k] = g.bits;
      const BitString u = lr_code_of_uv(rf, k); P.lr_code_len_uv[rf][k] = u.len; P.lr_code_bits_uv[rf][k] = u.bits;
    }
  return P;
}

}  // namespace

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

// The four streams of a context come from a process-wide pool and go back to it when the context is destroyed.  The runtime maps
// streams onto a few hardware queues in creation order, and after contexts had been created and destroyed a number of times a new
// context's chain stream could share a queue with its own search stream, whose launches for the whole chunk are queued up front: a
// single 1080p IPPP chunk then took 20.3 ms instead of 13.7 (bench.py's configs run one after the other in one process; a daemon that
// lives for days is the same case).  Reused streams keep the mapping of the first contexts.
namespace {
struct StreamSet { hipStream_t s[4]; };
std::mutex g_stream_mu;
std::vector<std::pair<int, StreamSet>> g_stream_pool;   // (device, set)
}  // namespace
extern "C" void av1mi_host_release_streams(void) {
  std::vector<std::pair<int, StreamSet>> all;
  { std::lock_guard<std::mutex> lk(g_stream_mu); all.swap(g_stream_pool); }
  for (auto &e : all) {
    (void)hipSetDevice(e.first);
    for (auto st : e.second.s) if (st) (void)hipStreamDestroy(st);
  }
}

int av1mi_ctx_create(int device_id, av1mi_ctx **out) {
  if (!out) return AV1MI_E_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return AV1MI_E_NO_DEVICE;
  av1mi_ctx *c = new (std::nothrow) av1mi_ctx();
  if (!c) return AV1MI_E_OOM;
  c->device = device_id;
  // test hook: start at a capacity multiplier content would otherwise have to provoke (tests/test_gpu_parity.py: slots beyond 4 GB)
  if (const char *e = getenv("AV1MI_CAP_SCALE")) { const int k = atoi(e); if (k >= 1 && k <= 64 && (k & (k - 1)) == 0) c->cap_scale = k; }
  if (const char *e = getenv("AV1MI_SYM_ORDER")) c->sym_order = atoi(e) != 0;   // experiment knob: 0 = natural tile order in symbolize
  // the main stream carries the serial chain of a chunk (and the latency-bound range coder): highest priority, so that
  // the bulk work put beside it on the second stream (CDEF, SSE, the chunk-wide motion search) fills gaps instead of
  // taking its slots
  int prio_lo = 0, prio_hi = 0;
  if (hipSetDevice(device_id) == hipSuccess) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  bool pooled = false;   // a pooled set, if there is one for this device
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (size_t i = 0; i < g_stream_pool.size(); i++)
      if (g_stream_pool[i].first == device_id) {
        const StreamSet ss = g_stream_pool[i].second;
        g_stream_pool.erase(g_stream_pool.begin() + (long)i);
        c->stream = ss.s[0]; c->stream2 = ss.s[1]; c->stream3 = ss.s[2]; c->stream4 = ss.s[3];
        pooled = true;
        break;
      }
  }
  if (pooled) {
    if (hipSetDevice(device_id) != hipSuccess) { delete c; return AV1MI_E_NO_DEVICE; }
  } else
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_lo) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio_lo) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream4, hipStreamNonBlocking, prio_lo) != hipSuccess) {
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    if (c->stream4) (void)hipStreamDestroy(c->stream4);
    delete c;
    return AV1MI_E_NO_DEVICE;
  }
  for (auto &e : c->ev) (void)hipEventCreate(&e);
  *out = c;
  return AV1MI_OK;
}

void av1mi_ctx_destroy(av1mi_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  free_workspace(c);
  for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
  for (auto &e : c->me_ev) (void)hipEventDestroy(e);
  for (auto &e : c->grp_ev) (void)hipEventDestroy(e);
  (void)hipStreamSynchronize(c->stream2); (void)hipStreamSynchronize(c->stream3); (void)hipStreamSynchronize(c->stream4);
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    g_stream_pool.push_back({ c->device, StreamSet{ { c->stream, c->stream2, c->stream3, c->stream4 } } });
  }
  delete c;
}

// A context that goes back to av1mi_encode_file's cache forgets the capacity multiplier its last job's content raised (it would
// otherwise size - or, at the limit, refuse - an unrelated job's workspace by it); the next chunk reallocates at scale 1.
void av1mi_host_ctx_recycle(av1mi_ctx *c) { if (c) c->cap_scale = 1; }

const char *av1mi_last_error(const av1mi_ctx *c) { return c ? c->err.c_str() : "no context"; }

// Bitstream buffers handed to the caller (av1mi_buf.data) are page-locked blocks from a process-wide pool: the packed chunk is
// copied device -> host straight into the block the caller gets, and av1mi_free() puts the block back for the next chunk - no
// staging copy and no first-touch page faults on a fresh malloc per chunk (2.35 MB per 1080p all-key-frame chunk, 23 MB at the
// production point: 0.2 / 1.1 ms of host time per chunk before).  Blocks that do not come from the pool are plain malloc.
namespace {
std::mutex g_pin_mu;
std::vector<std::pair<void *, size_t>> g_pin_out;    // handed out: (block, capacity)
std::vector<std::pair<void *, size_t>> g_pin_free;   // waiting for the next chunk
constexpr size_t PIN_FREE_MAX_BYTES = (size_t)1 << 30;
// parked blocks: a job with w workers has up to 2 w finished chunks waiting for the writer, so the bound follows the largest worker
// count seen (av1mi_host_expect_blocks) - freeing a block is hipHostFree, which synchronises the whole device
std::atomic<size_t> g_pin_free_max_blocks{16};

void *pin_acquire(size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    int best = -1;
    for (size_t i = 0; i < g_pin_free.size(); i++)
      if (g_pin_free[i].second >= bytes && (best < 0 || g_pin_free[i].second < g_pin_free[(size_t)best].second)) best = (int)i;
    if (best >= 0) {
      const std::pair<void *, size_t> b = g_pin_free[(size_t)best];
      g_pin_free.erase(g_pin_free.begin() + best);
      g_pin_out.push_back(b);
      return b.first;
    }
  }
  void *p = nullptr;
  const size_t cap = bytes + (bytes >> 2) + 4096;
  if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_out.emplace_back(p, cap);
  return p;
}
}  // namespace

extern "C" void av1mi_host_expect_blocks(unsigned n) {
  size_t cur = g_pin_free_max_blocks.load();
  while (n > cur && n <= 256 && !g_pin_free_max_blocks.compare_exchange_weak(cur, n)) { }
}

extern "C" void av1mi_host_release_buffers(void) {
  std::vector<std::pair<void *, size_t>> all;
  { std::lock_guard<std::mutex> lk(g_pin_mu); all.swap(g_pin_free); }
  for (auto &b : all) (void)hipHostFree(b.first);
}

void av1mi_free(void *p) {
  if (!p) return;
  bool pooled = false, drop = false;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pin_out.size(); i++)
      if (g_pin_out[i].first == p) {
        const std::pair<void *, size_t> b = g_pin_out[i];
        g_pin_out.erase(g_pin_out.begin() + (long)i);
        size_t held = 0;
        for (auto &f : g_pin_free) held += f.second;
        if (g_pin_free.size() < g_pin_free_max_blocks.load() && held + b.second <= PIN_FREE_MAX_BYTES) g_pin_free.push_back(b);
        else drop = true;
        pooled = true;
        break;
      }
  }
  if (!pooled) free(p);
  else if (drop) (void)hipHostFree(p);
}

// Scene-cut rule (include/av1mi.h: av1mi_scene_cuts).  Integer only: d = mean absolute luma difference at 8-bit
// scale in Q8.  Mirrored by oracle/scenecut.py.
static int scene_rule_step(av1mi_scene_state *st, int has_prev, uint64_t sad, uint64_t luma_samples, int bit_depth, uint32_t min_len) {
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

int av1mi_scene_cuts(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                     const void *prev_frame, av1mi_scene_state *state, uint32_t min_scene_len, uint64_t *sad_out, uint8_t *is_cut) {
  if (!c || !frames || !state || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Resolved r;
  int rc = resolve(params, &r);
  if (rc) { set_err(c, "invalid parameters"); return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  const int bps = r.p.bit_depth > 8 ? 2 : 1;
  const size_t frame_bytes = caller_bytes(r, 1);
  Av1miDevParams P;
  memset(&P, 0, sizeof(P));
  P.width = r.p.width; P.height = r.p.height; P.bit_depth = r.p.bit_depth; P.n_frames = (int)n_frames;  // tight input layout
  P.true_w = P.width; P.true_h = P.height;
  P.frame_samples = (long)(frame_bytes / bps);
  hipStream_t s = c->stream;
  // host input: stage [prev | frames] contiguously on the device (frame_bytes is a multiple of 32)
  void *d_stage = nullptr;
  unsigned long long *d_sad = nullptr;
  const uint8_t *d_frames, *d_prev = nullptr;
  auto cleanup = [&] { if (d_stage) (void)hipFree(d_stage); if (d_sad) (void)hipFree(d_sad); };
  hipError_t e = hipMalloc((void **)&d_sad, (size_t)n_frames * 8);
  if (e == hipSuccess) e = hipMemsetAsync(d_sad, 0, (size_t)n_frames * 8, s);
  if (e == hipSuccess && !frames_on_device) {
    e = hipMalloc(&d_stage, (size_t)(n_frames + 1) * frame_bytes);
    if (e == hipSuccess && prev_frame) e = hipMemcpyAsync(d_stage, prev_frame, frame_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync((uint8_t *)d_stage + frame_bytes, frames, (size_t)n_frames * frame_bytes, hipMemcpyHostToDevice, s);
    d_frames = (const uint8_t *)d_stage + frame_bytes;
    d_prev = prev_frame ? (const uint8_t *)d_stage : nullptr;
  } else {
    d_frames = (const uint8_t *)frames;
    d_prev = (const uint8_t *)prev_frame;
    if (((uintptr_t)d_frames | (uintptr_t)d_prev) & 15) { cleanup(); set_err(c, "device frames must be 16-byte aligned"); return AV1MI_E_INVALID_ARG; }
  }
  std::vector<unsigned long long> sad(n_frames, 0);
  if (e == hipSuccess) e = av1mi_launch_luma_sad(&P, d_frames, d_prev, d_sad, s);
  if (e == hipSuccess) e = hipMemcpyAsync(sad.data(), d_sad, (size_t)n_frames * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  cleanup();
  if (e != hipSuccess) { set_err(c, "scene-cut pass failed: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP; }
  const uint64_t luma = (uint64_t)r.p.width * r.p.height;
  for (uint32_t t = 0; t < n_frames; t++) {
    const int has_prev = t > 0 || prev_frame != nullptr;
    const int cut = scene_rule_step(state, has_prev, sad[t], luma, (int)r.p.bit_depth, min_scene_len ? min_scene_len : 1);
    if (is_cut) is_cut[t] = (uint8_t)cut;
    if (sad_out) sad_out[t] = sad[t];
  }
  return AV1MI_OK;
}

// The adaptive quantisation's decision alone: the same two launches the encoder runs on a chunk's source (av1mi_launch_aq), on buffers of
// the call's own.
int av1mi_aq_qindex(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, uint8_t *qindex) {
  if (!c || !frames || !qindex || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Resolved r;
  int rc = resolve(params, &r);
  if (rc) { set_err(c, "invalid parameters"); return rc; }
  const size_t nsb = (size_t)r.sb_cols * r.sb_rows, n_map = (size_t)n_frames * nsb;
  if (!r.aq) { memset(qindex, r.qidx, n_map); return AV1MI_OK; }
  if (frames_on_device && ((uintptr_t)frames & 15)) { set_err(c, "device frames must be 16-byte aligned"); return AV1MI_E_INVALID_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  const int bps = r.p.bit_depth > 8 ? 2 : 1;
  const size_t in_bytes = caller_bytes(r, n_frames), coded_bytes = (size_t)n_frames * r.cw * r.ch * 3 / 2 * bps;
  const Av1miDevParams P = dev_params(r, n_frames, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hipStream_t s = c->stream;
  void *d_in = nullptr, *d_coded = nullptr;
  uint16_t *d_act = nullptr;
  uint8_t *d_map = nullptr;
  auto cleanup = [&] { for (void *b : { d_in, d_coded, (void *)d_act, (void *)d_map }) if (b) (void)hipFree(b); };
  hipError_t e = hipMalloc((void **)&d_act, n_map * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc((void **)&d_map, n_map);
  const void *src = frames;
  if (e == hipSuccess && !frames_on_device) {
    e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, frames, in_bytes, hipMemcpyHostToDevice, s);
    src = d_in;
  }
  if (e == hipSuccess && r.padded) {   // the rule reads the coded size: edge-extended as the encoder's source is
    e = hipMalloc(&d_coded, coded_bytes);
    if (e == hipSuccess) e = av1mi_launch_pad(src, d_coded, (int)r.p.width, (int)r.p.height, r.cw, r.ch, (int)r.p.bit_depth, (int)n_frames, 0, s);
    src = d_coded;
  }
  if (e == hipSuccess) e = av1mi_launch_aq(&P, src, d_act, d_map, r.aq, s);
  if (e == hipSuccess) e = hipMemcpyAsync(qindex, d_map, n_map, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);   // (also after a failure: nothing may still read the buffers freed below)
  cleanup();
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { set_err(c, "adaptive-quantisation pass failed: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP; }
  return AV1MI_OK;
}

// The temporal filter alone: the launch the encoder runs on a chunk's source (av1mi_launch_temporal_filter), on buffers of the call's own.
int av1mi_temporal_filter(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, void *out,
                          uint32_t *mv) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Resolved r;
  int rc = resolve(params, &r);
  if (rc) { set_err(c, "invalid parameters"); return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  const int bps = r.p.bit_depth > 8 ? 2 : 1;
  const size_t in_bytes = caller_bytes(r, n_frames), coded_bytes = (size_t)n_frames * r.cw * r.ch * 3 / 2 * bps;
  const size_t n_mv = tf_mv_entries(r, n_frames);
  const Av1miDevParams P = dev_params(r, n_frames, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hipStream_t s = c->stream;
  const hipMemcpyKind in_kind = frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, out_kind = frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  void *d_in = nullptr, *d_coded = nullptr;   // the frames as the caller has them (padded sizes: in, then the cropped result), and at the coded size
  uint32_t *d_mv = nullptr;
  auto cleanup = [&] { for (void *b : { d_in, d_coded, (void *)d_mv }) if (b) (void)hipFree(b); };
  hipError_t e = hipMalloc(&d_coded, coded_bytes);
  if (e == hipSuccess && n_mv) e = hipMalloc((void **)&d_mv, n_mv * sizeof(uint32_t));
  if (e == hipSuccess && r.padded) {   // edge-extended as the encoder's source is
    const void *src = frames;
    e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess && !frames_on_device) { e = hipMemcpyAsync(d_in, frames, in_bytes, hipMemcpyHostToDevice, s); src = d_in; }
    if (e == hipSuccess) e = av1mi_launch_pad(src, d_coded, (int)r.p.width, (int)r.p.height, r.cw, r.ch, (int)r.p.bit_depth, (int)n_frames, 0, s);
  } else if (e == hipSuccess) {
    e = hipMemcpyAsync(d_coded, frames, in_bytes, in_kind, s);
  }
  if (e == hipSuccess && n_mv) e = av1mi_launch_temporal_filter(&P, d_coded, d_mv, r.tf_frames, r.tf_strength, s);
  if (e == hipSuccess && out) {
    const void *res = d_coded;
    if (r.padded) {
      e = av1mi_launch_pad(d_coded, d_in, (int)r.p.width, (int)r.p.height, r.cw, r.ch, (int)r.p.bit_depth, (int)n_frames, 1, s);
      res = d_in;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, res, in_bytes, out_kind, s);
  }
  if (e == hipSuccess && mv && n_mv) e = hipMemcpyAsync(mv, d_mv, n_mv * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);   // (also after a failure: nothing may still read the buffers freed below)
  cleanup();
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { set_err(c, "temporal-filter pass failed: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP; }
  return AV1MI_OK;
}

// The levels the context's last chunk was deblocked with and, with the level search, the candidates' errors: what download_chunk kept.
int av1mi_lf_search_result(const av1mi_ctx *c, uint32_t n_frames, uint8_t *levels, uint64_t *err) {
  if (!c || !levels || n_frames == 0 || c->lf_levels.size() != (size_t)n_frames * 4) return AV1MI_E_INVALID_ARG;
  memcpy(levels, c->lf_levels.data(), c->lf_levels.size());
  if (err) memcpy(err, c->lf_errs.data(), c->lf_errs.size() * sizeof(unsigned long long));
  return AV1MI_OK;
}

static int encode_chunk_once(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                             av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report);

int av1mi_encode_chunk(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                       av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report) {
  if (!c || !frames || !out || n_frames == 0) return AV1MI_E_INVALID_ARG;
  for (;;) {
    const int rc = encode_chunk_once(c, params, frames, n_frames, frames_on_device, out, frame_sizes, recon, report);
    if (rc != AV1MI_E_OVERFLOW || c->cap_scale >= 64) return rc;
    c->cap_scale *= 2;  // stays raised for the following chunks of this context (same content)
  }
}

uint32_t av1mi_lr_fit_units(const av1mi_ctx *c) { return c ? c->fit_plane_units : 0; }
// The self-guided fit of the context's last chunk: what download_chunk fetched, zeros for a chunk without the fit.
int av1mi_lr_fit_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *units, uint64_t *err) {
  if (!c || !units || n_frames == 0 || c->lf_levels.size() != (size_t)n_frames * 4) return AV1MI_E_INVALID_ARG;
  const size_t n = c->fit_units;
  if (c->fit_on) {
    const Av1miLrFit H = av1mi_lr_fit_split(c->ws.h_fit, n, 0);   // the fetched head of the block
    memcpy(units, H.rec, n * 4);
    if (err) memcpy(err, H.err, n * AV1MI_LR_FIT_CANDS * 8);
  } else {
    memset(units, 0, n * 4);
    if (err) memset(err, 0, n * AV1MI_LR_FIT_CANDS * 8);
  }
  return AV1MI_OK;
}

// The order symbolize took the last chunk's tiles in: the classes' counters and rows as they still stand on the device (the next chunk's
// prepare_chunk clears them), fetched here - not with the chunk's small results, it is a diagnostic.
int av1mi_sym_order_result(const av1mi_ctx *c, uint32_t *order, uint8_t *classes, uint32_t n) {
  if (!c || !order || !classes || c->lf_levels.empty() || n != c->sym_tiles || n == 0) return AV1MI_E_INVALID_ARG;
  uint32_t count[AV1MI_TILE_CLASSES];
  if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(count, c->ws.d_sym_count, sizeof(count), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  uint32_t at = 0;
  for (int k = AV1MI_TILE_CLASSES - 1; k >= 0; k--) {
    if (count[k] > n - at) return AV1MI_E_HIP;   // (the counters do not add up to the chunk's tiles)
    if (count[k] && hipMemcpy(order + at, c->ws.d_sym_order + (size_t)k * n, (size_t)count[k] * 4, hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
    for (uint32_t i = 0; i < count[k]; i++) {
      if (order[at + i] >= n) return AV1MI_E_HIP;
      classes[order[at + i]] = (uint8_t)k;
    }
    at += count[k];
  }
  return at == n ? AV1MI_OK : AV1MI_E_HIP;
}
uint32_t av1mi_sym_order_tiles(const av1mi_ctx *c) { return c && !c->lf_levels.empty() ? c->sym_tiles : 0; }

// The partition of the last chunk's frames and the integer search's keys, as they still stand on the device (the context's next chunk
// overwrites them), fetched here - a diagnostic like av1mi_sym_order_result.
uint32_t av1mi_inter_partition_units(const av1mi_ctx *c) { return c && c->pi_frames ? c->pi_units : 0; }
int av1mi_inter_partition_result(const av1mi_ctx *c, uint32_t n_frames, uint32_t *masks, uint64_t *keys) {
  if (!c || !masks || !keys || n_frames == 0 || c->pi_frames != n_frames || c->lf_levels.empty()) return AV1MI_E_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return AV1MI_E_HIP;
  if (hipMemcpy(masks, c->ws.d_part, (size_t)n_frames * c->pi_sbs * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  // (the keys are the node-mode search's: a chunk without it - partition_search = 1, or no inter frame - reports zeros)
  if (!c->pi_keys) memset(keys, 0, (size_t)n_frames * c->pi_units * sizeof(uint64_t));
  else if (hipMemcpy(keys, c->ws.d_me, (size_t)n_frames * c->pi_units * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  return AV1MI_OK;
}

uint32_t av1mi_lr_wiener_fit_units(const av1mi_ctx *c) { return c ? c->fit_plane_units : 0; }
// The Wiener fit of the context's last chunk, likewise.
int av1mi_lr_wiener_fit_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *units, uint64_t *err) {
  if (!c || !units || n_frames == 0 || c->lf_levels.size() != (size_t)n_frames * 4) return AV1MI_E_INVALID_ARG;
  const size_t n = c->fit_units;
  if (c->wfit_on) {
    const Av1miLrWfit H = av1mi_lr_wfit_split(c->ws.h_wfit, n);   // the fetched head of the block
    memcpy(units, H.rec, n * 8);
    if (err) memcpy(err, H.err, n * 8);
  } else {
    memset(units, 0, n * 8);
    if (err) memset(err, 0, n * 8);
  }
  return AV1MI_OK;
}

uint32_t av1mi_lr_rd_units(const av1mi_ctx *c) { return c ? c->fit_plane_units : 0; }
// The final restoration decisions of the context's last chunk: the choices as they still stand on the device (the context's next chunk
// overwrites them), fetched here - a diagnostic like av1mi_sym_order_result - and their B16 from the fits' records, which arrived with
// the chunk.
int av1mi_lr_rd_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *choice, uint32_t *bits16, uint64_t *lambda) {
  if (!c || !choice || n_frames == 0 || c->lf_levels.size() != (size_t)n_frames * 4) return AV1MI_E_INVALID_ARG;
  const Av1miDevParams &P = c->P;
  const size_t n = c->fit_units, per = c->fit_plane_units;
  memset(choice, 0, n);
  if (bits16) memset(bits16, 0, n * sizeof(uint32_t));
  if (lambda) *lambda = P.enable_lr ? P.lr_lambda : 0;
  if (!P.enable_lr) return AV1MI_OK;
  const int planes = P.lr_chroma ? 3 : 1, sw = P.enable_lr == 2;
  std::vector<uint8_t> dev((size_t)n_frames * planes * per);   // [frame][restored plane][unit]
  if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(dev.data(), c->ws.d_lrc, dev.size(), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  const Av1miLrFit G = c->fit_on ? av1mi_lr_fit_split(c->ws.h_fit, n, 0) : Av1miLrFit{};
  const Av1miLrWfit W = c->wfit_on ? av1mi_lr_wfit_split(c->ws.h_wfit, n) : Av1miLrWfit{};
  for (uint32_t f = 0; f < n_frames; f++)
    for (int pl = 0; pl < planes; pl++)
      for (size_t k = 0; k < per; k++) {
        const size_t u = ((size_t)f * 3 + pl) * per + k;
        const int ch = dev[((size_t)f * planes + pl) * per + k];
        choice[u] = (int8_t)ch;
        if (!bits16) continue;
        int lc = 0;
        if (ch == AV1MI_LR_WFIT_CHOICE) {
          if (!W.rec) return AV1MI_E_HIP;
          const int8_t *q = W.rec + u * 8;
          lc = av1mi_lr_wiener_lc(pl > 0, q[2], q[3], q[4], q[5], q[6], q[7]);
        } else if (ch >= 7) {
          if (!G.rec) return AV1MI_E_HIP;
          const int8_t *q = G.rec + u * 4;
          lc = av1mi_lr_sgr_lc(q[1], q[2], q[3]);
        } else if (ch >= 4) lc = P.sgr_code_len[0][ch - 4];
        else if (ch) lc = pl ? P.lr_code_len_uv[0][ch - 1] : P.lr_code_len[0][ch - 1];
        bits16[u] = (uint32_t)av1mi_lr_b16(lc, av1mi_lr_type_t16(sw, av1mi_lr_choice_type(ch)));
      }
  return AV1MI_OK;
}

// ---- one chunk: prepare_chunk, the schedule of its kind with entropy coding inside, packing, download_chunk
// Header blob, CDFs, parameters and clears, then the source frames - uploaded, and edge-extended where the coded size is not the
// signalled one - and their partition.  *d_src: the chunk's source frames on the device, at the coded size.
static int prepare_chunk(av1mi_ctx *c, const Resolved &r, const void *frames, uint32_t n_frames, int frames_on_device, const void **d_src) {
  Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream;
  // header blob: sequence header OBU, then one fixed-size slot per frame with that frame's header (key and inter
  // frames have different lengths; frames of one kind differ only in grain_seed)
  size_t str_key = 0, str_inter = 0;   // CDEF strength search: where cdef_select_kernel writes each frame's set
  size_t lf_key = 0, lf_inter = 0;     // deblocking level search: where deblock_decide_kernel writes each frame's levels
  std::vector<uint8_t> seq = make_sequence_header(r), fh = make_frame_header(r, nullptr, 0, false, &str_key, &lf_key),
                       fhi = make_frame_header(r, nullptr, 0, true, &str_inter, &lf_inter);
  P.cdef_str_bit[0] = (int)str_key; P.cdef_str_bit[1] = (int)str_inter;
  P.lf_bit[0] = (int)lf_key; P.lf_bit[1] = (int)lf_inter;
  P.seq_hdr_bytes = (int)seq.size(); P.frame_hdr_bytes = (int)fh.size(); P.inter_hdr_bytes = (int)fhi.size();
  if (seq.size() > 256 || fh.size() > (size_t)P.hdr_slot_bytes || fhi.size() > (size_t)P.hdr_slot_bytes) { set_err(c, "internal: header larger than its slot"); return AV1MI_E_OVERFLOW; }
  std::vector<uint8_t> blob(seq.size() + (size_t)n_frames * P.hdr_slot_bytes, 0);
  memcpy(blob.data(), seq.data(), seq.size());
  for (uint32_t f = 0; f < n_frames; f++) {
    const bool inter = av1mi_frame_is_inter(P, (int)f);
    std::vector<uint8_t> &h = inter ? fhi : fh;
    if (r.p.film_grain && f) h = make_frame_header(r, nullptr, f, inter);
    memcpy(blob.data() + seq.size() + (size_t)f * P.hdr_slot_bytes, h.data(), h.size());
  }
  // Upload what the device does not hold already (consecutive chunks of a job: nothing), from page-locked memory - the copies are
  // asynchronous, and the previous chunk's have completed (download_chunk waits for the main stream).  With the strength search on,
  // cdef_select_kernel writes the strengths into the frame headers on the device: the blob goes up every chunk.  Likewise with the
  // deblocking level search (deblock_decide_kernel writes the levels).
  if (w.hdr_bytes != blob.size() || memcmp(w.h_hdr, blob.data(), blob.size())) {
    w.hdr_bytes = 0;
    memcpy(w.h_hdr, blob.data(), blob.size());
    HIPCHK(c, hipMemcpyAsync(w.d_hdr, w.h_hdr, blob.size(), hipMemcpyHostToDevice, s));
  }
  w.hdr_bytes = P.cdef_search || P.lf_search ? 0 : blob.size();
  if (w.cdf_qidx != r.qidx || w.cdf_bs_log2 != P.max_bs_log2) {
    w.cdf_qidx = -1;
    // the blob, and behind it the regular symbolize variants' compact image of it for this leaf size (av1mi_dev.h: Av1miCdfCompact)
    std::vector<uint16_t> cdf = make_cdf_blob(r.qidx);
    cdf.resize(Av1miCdfCompact::BLOB_WORDS, 0);
    av1mi_cdf_compact_build(cdf.data(), P.max_bs_log2, cdf.data() + Av1miCdfCompact::AT);
    memcpy(w.h_cdf, cdf.data(), cdf.size() * 2);
    HIPCHK(c, hipMemcpyAsync(w.d_cdf, w.h_cdf, cdf.size() * 2, hipMemcpyHostToDevice, s));
    w.cdf_qidx = r.qidx; w.cdf_bs_log2 = P.max_bs_log2;
  }
  {
    // The recon kernel reads its parameters from device memory.  With adaptive quantisation the block is followed by one copy per
    // quantiser slot (av1mi_aq_slot) that differs in the quantiser steps, their reciprocals and the quantiser-matrix slice alone: the
    // walk takes its superblock's copy, and everything else it reads there is what the first block holds.
    const int n_par = P.aq_map ? AV1MI_AQ_SLOTS : 1;
    std::vector<Av1miDevParams> par((size_t)n_par, P);
    for (int sl = 1; sl < n_par; sl++) {
      Av1miDevParams &Q = par[(size_t)sl];
      set_quant_steps(Q, quant_steps(av1mi_aq_slot_qindex(sl, r.qidx), P.bit_depth));
      if (P.qm_tab) Q.qm_tab = P.qm_tab + (size_t)sl * 2 * AV1MI_QM_PLANE;
    }
    const size_t bytes = (size_t)n_par * sizeof(P);
    if (w.params_on_device < n_par || memcmp(w.h_params, par.data(), bytes)) {   // (dev_params clears the padding; a cap_scale change shows in P)
      w.params_on_device = 0;
      memcpy(w.h_params, par.data(), bytes);
      HIPCHK(c, hipMemcpyAsync(w.d_params, w.h_params, bytes, hipMemcpyHostToDevice, s));
      w.params_on_device = n_par;
    }
  }
  HIPCHK(c, hipMemsetAsync(w.d_record, 0, sizeof(Av1miChunkRecord), s));
  HIPCHK(c, hipMemsetAsync(w.d_sym_count, 0, AV1MI_TILE_CLASSES * 4 + (size_t)n_frames * 24, s));   // the classes' counters and d_sse behind them
  if (P.cdef_search) HIPCHK(c, hipMemsetAsync(w.d_cdef_err, 0, (size_t)n_frames * P.sb_rows * P.sb_cols * 24 * sizeof(unsigned long long), s));
  // the level search's sums, once per attempt at the chunk (not a fill per frame on a P chain)
  if (P.lf_search) HIPCHK(c, hipMemsetAsync(w.d_lf_err, 0, (size_t)n_frames * 3 * AV1MI_LF_CANDS * sizeof(unsigned long long), s));
  // the self-guided fit's sums, errors, records and codes, once per attempt at the chunk
  if (P.lr_fit_code) HIPCHK(c, hipMemsetAsync(w.d_fit, 0, av1mi_lr_fit_bytes(fit_chunk_units(r, n_frames)), s));
  if (P.lr_wfit_code) HIPCHK(c, hipMemsetAsync(w.d_wfit, 0, av1mi_lr_wfit_bytes(fit_chunk_units(r, n_frames)), s));
  HIPCHK(c, hipEventRecord(c->ev[EV_START], s));
  // the caller's frames are used in place if they are on the device at the coded size; a padded chunk arrives in the stage
  if (!frames_on_device) HIPCHK(c, hipMemcpyAsync(r.padded ? w.d_stage : w.d_src, frames, caller_bytes(r, n_frames), hipMemcpyHostToDevice, s));
  // not a multiple of 8: edge-extend every frame to the coded size (the signalled size stays exact)
  if (r.padded) HIPCHK(c, av1mi_launch_pad(frames_on_device ? frames : w.d_stage, w.d_src, (int)r.p.width, (int)r.p.height, r.cw, r.ch, P.bit_depth, (int)n_frames, 0, s));
  *d_src = frames_on_device && !r.padded ? frames : w.d_src;
  // the key frames' temporal filter: in place in the chunk's source - a chunk that is used in place is copied first, the caller's
  // memory is never written.  Everything below and after reads the filtered key frames.
  if (tf_runs(r, n_frames)) {
    if (*d_src != w.d_src) { HIPCHK(c, hipMemcpyAsync(w.d_src, frames, caller_bytes(r, n_frames), hipMemcpyDeviceToDevice, s)); *d_src = w.d_src; }
    HIPCHK(c, av1mi_launch_temporal_filter(&P, w.d_src, w.d_tf_mv, r.tf_frames, r.tf_strength, s));
  }
  // content-driven partition: the split masks of every superblock of the chunk, from the source, before anything walks blocks (the second
  // stream's motion search waits for EV_SRC_READY as well)
  if (P.part_map) HIPCHK(c, av1mi_launch_partition(&P, *d_src, w.d_part, s));
  // adaptive quantisation: every superblock's quantiser index, likewise from the source and on the device - the walks and symbolize read the map
  if (P.aq_map) HIPCHK(c, av1mi_launch_aq(&P, *d_src, w.d_aq_act, w.d_aq_map, r.aq, s));
  HIPCHK(c, hipEventRecord(c->ev[EV_SRC_READY], s));
  return AV1MI_OK;
}

// Whether symbolize takes this chunk's tiles heavy first: all-key-frame chunks with one-superblock tiles, adaptive CDFs and
// leaves up to 32x32, unless AV1MI_SYM_ORDER = 0.  The reconstruction launch then fills the table and symbolize reads it; sym_tiles
// remembers it for av1mi_sym_order_result.  (64x64 leaves: measured, the reconstruction wave's wait for its place in the table - it
// has just stored a whole superblock - costs that launch 0.034 ms, more than symbolize gains: DESIGN 5h.)
static bool sym_order_on(av1mi_ctx *c, uint32_t n_frames) {
  const bool on = c->sym_order && c->P.tile_sb == 1 && !c->P.disable_cdf_update && c->P.max_bs_log2 <= 5;
  c->sym_tiles = on ? n_frames * (uint32_t)(c->P.tile_rows * c->P.tile_cols) : 0;
  return on;
}

// Entropy coding of frames [from, n_frames) on the main stream (the frame-edge tiles' symbolize variant on the fourth), then the join
// with the groups of frames before `from` coded on the third (schedule_inter): packing needs the tile sizes and bytes of every frame.
// by_weight: symbolize takes the tiles in the order the chunk's reconstruction launch left (sym_order_on).
static int entropy_code(av1mi_ctx *c, uint32_t from, uint32_t n_frames, bool by_weight = false) {
  Workspace &w = c->ws; hipStream_t s = c->stream;
  HIPCHK(c, hipEventRecord(c->ev[EV_RECON_DONE], s));
  HIPCHK(c, av1mi_launch_entropy(&c->P, w.d_cdf, w.d_levels, w.d_blk, w.d_streams, w.d_sym, w.d_combos, w.d_slots, w.d_tile_bytes, w.d_lrc,
                                 w.d_tile_off /* scratch until the packing kernels fill it */, by_weight ? w.d_sym_count : nullptr,
                                 by_weight ? w.d_sym_order : nullptr, (int)from, (int)(n_frames - from),
                                 s, c->ev[EV_SYM_DONE], c->stream4, c->ev[EV_EDGE_FORK], c->ev[EV_EDGE_JOIN]));
  if (from) HIPCHK(c, hipStreamWaitEvent(s, c->ev[EV_GROUPS_JOINED], 0));
  HIPCHK(c, hipEventRecord(c->ev[EV_ENTROPY_DONE], s));
  return AV1MI_OK;
}

// The second stream beside the range coder, once symbolize is done: the squared error of the final frames
static int sse_beside_range_coder(av1mi_ctx *c, const void *src) {
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev[EV_SYM_DONE], 0));
  HIPCHK(c, hipEventRecord(c->ev[EV_CDEF_START], c->stream2));
  HIPCHK(c, av1mi_launch_sse(&c->P, src, c->ws.d_fin, c->ws.d_sse, c->stream2));
  HIPCHK(c, hipEventRecord(c->ev[EV_CDEF_DONE], c->stream2));
  return AV1MI_OK;
}

// All-key-frame chunk: one reconstruction launch over the chunk.  The frames are independent, so the chunk could run as a software
// pipeline over groups of frames - the main stream reconstructing group g + 1 while auxiliary streams symbolize and range-code group
// g.  Measured (1080p x 60, MI355X): 14.1 k frames/s as one group, 12.3 k as two, 10.7 k as three - the range coder holds 145 KB of
// LDS on every CU it sits on, which leaves the reconstruction (10 KB per wave) one wave there instead of sixteen.
// CDEF (+SSE) depends only on the reconstruction.  The range-coding kernel is a latency-bound serial chain (one lane per tile: 480
// waves, half the SIMDs idle), so CDEF runs beside IT on the second stream; symbolize and CDEF are both throughput-bound and would
// only slow each other.
static int schedule_all_key(av1mi_ctx *c, const void *src, uint32_t n_frames) {
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream, s2 = c->stream2;
  // Deblocking reads only the reconstruction and block info: beside symbolize on the second stream.  The strength search reads the
  // deblocked frames and symbolize codes its cdef_idx: with the search on, deblocking and search run before entropy coding.  So they do
  // with the deblocking level search, whose decision writes into the headers the main stream packs.
  const hipStream_t deblock_s = P.cdef_search || P.lf_search ? s : s2;
  // CDEF's one launch over the chunk sums the squared error itself - a second pass over the frames, 0.19 ms at 1080p x 60, would end
  // after the range coder CDEF runs beside; a one-frame chunk's CDEF runs in strips without the sum
  const bool sse_in_cdef = n_frames > 1;
  const bool deblock = av1mi_frame_lf_levels(P, 0)[0] != 0;
  const int n = (int)n_frames;
  const bool by_weight = sym_order_on(c, n_frames);
  HIPCHK(c, av1mi_launch_recon(&P, w.d_params, src, w.d_rec, w.d_levels, w.d_blk, nullptr, nullptr, 0, n, by_weight ? w.d_sym_count : nullptr,
                               by_weight ? w.d_sym_order : nullptr, s));
  if (P.lf_search) HIPCHK(c, av1mi_launch_deblock_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, 0, n, s));
  if (deblock && deblock_s == s) HIPCHK(c, av1mi_launch_deblock(&P, w.d_rec, w.d_blk, 0, n, s));
  if (P.cdef_search) HIPCHK(c, av1mi_launch_cdef_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, 0, n, s));
  if (const int rc = entropy_code(c, 0, n_frames, by_weight)) return rc;
  HIPCHK(c, hipStreamWaitEvent(s2, c->ev[EV_RECON_DONE], 0));
  if (deblock && deblock_s == s2) HIPCHK(c, av1mi_launch_deblock(&P, w.d_rec, w.d_blk, 0, n, s2));
  // measured: starting CDEF right after the reconstruction, beside symbolize, costs 8 % overall
  HIPCHK(c, hipStreamWaitEvent(s2, c->ev[EV_SYM_DONE], 0));
  HIPCHK(c, hipEventRecord(c->ev[EV_CDEF_START], s2));
  HIPCHK(c, av1mi_launch_cdef(&P, w.d_rec, w.d_fin, w.d_blk, sse_in_cdef ? src : nullptr, sse_in_cdef ? w.d_sse : nullptr, 0, n, s2));
  if (!sse_in_cdef) HIPCHK(c, av1mi_launch_sse(&P, src, w.d_fin, w.d_sse, s2));
  HIPCHK(c, hipEventRecord(c->ev[EV_CDEF_DONE], s2));
  return AV1MI_OK;
}

// Restoration of frames [frame0, frame0 + count) from `cdef` into d_fin: the fixed candidates - which also decide and filter unless the
// self-guided fit does - then the fits the chunk has.  clear: the launch clears its frames' unit sums (else the caller has)
static int launch_restoration(av1mi_ctx *c, const void *src, const void *cdef, int clear, int frame0, int count) {
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream;
  const Av1miLrFit *fit = P.lr_fit_code ? &w.fit : nullptr;
  HIPCHK(c, av1mi_launch_lr(&P, w.d_rec, cdef, src, w.d_fin, w.d_lrc, w.d_lrsse, clear, fit == nullptr, frame0, count, s));
  if (fit) HIPCHK(c, av1mi_launch_lr_fit(&P, w.d_rec, cdef, src, w.d_fin, w.d_lrc, w.d_lrsse, fit, frame0, count, s));
  if (P.lr_wfit_code) HIPCHK(c, av1mi_launch_lr_wfit(&P, w.d_rec, cdef, src, w.d_fin, w.d_lrc, w.d_lrsse, fit, &w.wfit, frame0, count, s));
  return AV1MI_OK;
}

// All-key-frame chunk with loop restoration: the unit decisions are part of the tile syntax, so deblocking, CDEF (into d_cd) and
// restoration (into d_fin) precede entropy coding on the main stream.
static int schedule_all_key_lr(av1mi_ctx *c, const void *src, uint32_t n_frames) {
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream;
  const int n = (int)n_frames;
  const bool by_weight = sym_order_on(c, n_frames);
  HIPCHK(c, av1mi_launch_recon(&P, w.d_params, src, w.d_rec, w.d_levels, w.d_blk, nullptr, nullptr, 0, n, by_weight ? w.d_sym_count : nullptr,
                               by_weight ? w.d_sym_order : nullptr, s));
  if (P.lf_search) HIPCHK(c, av1mi_launch_deblock_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, 0, n, s));
  if (av1mi_frame_lf_levels(P, 0)[0]) HIPCHK(c, av1mi_launch_deblock(&P, w.d_rec, w.d_blk, 0, n, s));
  if (P.cdef_search) HIPCHK(c, av1mi_launch_cdef_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, 0, n, s));
  HIPCHK(c, av1mi_launch_cdef(&P, w.d_rec, w.d_cd, w.d_blk, nullptr, nullptr, 0, n, s));
  int rc = launch_restoration(c, src, w.d_cd, 1, 0, n);
  if (!rc) rc = entropy_code(c, 0, n_frames, by_weight);
  return rc ? rc : sse_beside_range_coder(c, src);
}

// Inter chunk: a P frame needs the previous frame's final (post-CDEF) reconstruction, so reconstruction, deblocking, CDEF and
// restoration run frame by frame on the main stream; the motion search runs beside that chain on the second stream, entropy coding of
// finished groups of frames on the third (every frame starts from the default CDFs, so tiles of different frames stay independent).
static int schedule_inter(av1mi_ctx *c, const void *src, uint32_t n_frames) {
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream, s2 = c->stream2;
  const size_t nb8 = (size_t)P.b8_rows * P.b8_cols, nsb = (size_t)P.sb_rows * P.sb_cols;
  const bool lr = P.enable_lr != 0;
  void *cdef_out = lr ? w.d_cd : w.d_fin;   // with loop restoration CDEF writes d_cd and the restored frame goes to d_fin
  const unsigned long long *me_best = P.subpel ? w.d_me_sub : w.d_me;   // the keys the reconstruction reads
  // Motion search is open loop (source against previous source): all inter frames at once, on the second stream,
  // beside the chain below; the first inter frame's reconstruction waits for it.
  HIPCHK(c, hipStreamWaitEvent(s2, c->ev[EV_SRC_READY], 0));  // the source frames are in HBM
  HIPCHK(c, hipMemsetAsync(w.d_me, 0xFF, (size_t)n_frames * nb8 * 8, s2));
  uint32_t *acc64 = P.max_bs_log2 >= 6 ? w.d_me64 : nullptr;
  if (acc64) HIPCHK(c, hipMemsetAsync(acc64, 0, (size_t)n_frames * nsb * (2 * P.me_range + 1) * (2 * P.me_range + 1) * sizeof(uint32_t), s2));
  if (c->part_inter) HIPCHK(c, hipMemsetAsync(w.d_nodes, 0xFF, (size_t)n_frames * av1mi_pi_frame_nodes(P.b8_rows, P.b8_cols) * sizeof(uint32_t), s2));
  // one launch + one event per frame, enqueued from inside the frame loop below, behind the first frame's chain kernels: the chain's first
  // kernel (the key frame's reconstruction needs no vectors) no longer waits on the host for 120 - 180 API calls (under
  // the profiler the chain started 6.4 ms after the chunk's first kernel; unprofiled the calls take ~ 8 us each and one chunk gains nothing).
  // All of it behind the first frame rather than a few frames ahead of the chain - measured (1080p IPPP x 60, one chunk / four in flight,
  // frames/s): all 5 420 / 7 560; 8 ahead 5 390 / 7 220; 4 ahead 5 410 / 6 970; 2 ahead 5 370 / 6 900 - with several chunks in flight a
  // search that is enqueued late competes with the other chunks' chains instead of filling their gaps.
  while (c->me_ev.size() < n_frames) { hipEvent_t e; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->me_ev.push_back(e); }
  // hierarchical search: the chunk's luma at a quarter of the resolution (one launch), then per frame the superblocks' search centres
  const uint32_t *centre = P.me_presearch ? w.d_centre : nullptr;
  if (centre) HIPCHK(c, av1mi_launch_quarter_luma(&P, src, w.d_quarter, s2));
  // Entropy coding beside the chain: every frame starts from the default CDFs, so a group of frames can be symbolized and
  // range-coded (third stream) as soon as its last frame is reconstructed (and, with restoration on, its unit choices are
  // known) while the chain reconstructs the following frames; only the last group's entropy coding is left after the chain.
  // (AV1MI_ENTROPY_GROUP=k: groups of k frames - tests force small groups on short chunks; 0 = no overlap)
  // Group size: since the chain's kernels got short (walk 76, inter pass 38 us per 1080p frame) a range-coder launch beside them costs
  // more than it hides - 60-frame chunks, groups of 10 / 20 / none: 5 320 / 5 450 / 5 530 frames/s for one chunk, 7 670 / 8 050 / 7 970
  // with four in flight, 2 440 / 2 460 / 2 540 at the production point - so chunks of up to 64 frames code everything after the
  // chain and longer ones in groups of 32.
  uint32_t grp = n_frames <= 64 ? n_frames : 32;
  if (const char *eg = getenv("AV1MI_ENTROPY_GROUP")) { const int k = atoi(eg); grp = k > 0 ? (uint32_t)k : n_frames; }
  uint32_t n_grp = 0;
  // the restoration units' candidate sums of the whole chunk, cleared once (not a fill per frame on the chain)
  if (lr) HIPCHK(c, hipMemsetAsync(w.d_lrsse, 0, (size_t)n_frames * av1mi_lr_frame_units(P) * 8 * sizeof(unsigned long long), s));
  for (uint32_t f = 0; f < n_frames; f++) {
    const int fi = (int)f;
    if (av1mi_frame_is_inter(P, fi)) HIPCHK(c, hipStreamWaitEvent(s, c->me_ev[f], 0));
    HIPCHK(c, av1mi_launch_recon(&P, w.d_params, src, w.d_rec, w.d_levels, w.d_blk, w.d_fin, me_best, fi, 1, nullptr, nullptr, s));
    // the frame's levels before its deblocking (its reconstruction does not depend on them; everything after sees the chosen levels)
    if (P.lf_search) HIPCHK(c, av1mi_launch_deblock_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, fi, 1, s));
    if (av1mi_frame_lf_levels(P, fi)[0]) HIPCHK(c, av1mi_launch_deblock(&P, w.d_rec, w.d_blk, fi, 1, s));
    // the frame's strength set before its CDEF (the next frame's reference is the output of the chosen strengths)
    if (P.cdef_search) HIPCHK(c, av1mi_launch_cdef_search(&P, w.d_rec, src, w.d_blk, w.d_hdr, fi, 1, s));
    HIPCHK(c, av1mi_launch_cdef(&P, w.d_rec, cdef_out, w.d_blk, nullptr, nullptr, fi, 1, s));
    if (lr) { const int rc = launch_restoration(c, src, cdef_out, 0, fi, 1); if (rc) return rc; }
    if (f == 0)   // (frame 0 of a chunk is a key frame: its chain kernels are in the queue)
      for (uint32_t g = 1; g < n_frames; g++) {
        if (!av1mi_frame_is_inter(P, (int)g)) continue;
        if (centre) HIPCHK(c, av1mi_launch_presearch(&P, w.d_quarter, w.d_centre, (int)g, 1, s2));
        // partition_search = 2: the search keeps every node's best candidate, the decision writes the frame's masks and leaf keys
        if (c->part_inter) HIPCHK(c, av1mi_launch_inter_partition(&P, src, w.d_me, P.me_range, (int)g, 1, acc64, centre, w.d_nodes, w.d_part, s2));
        else HIPCHK(c, av1mi_launch_motion_search(&P, src, w.d_me, P.me_range, (int)g, 1, acc64, centre, s2));
        if (P.subpel) HIPCHK(c, av1mi_launch_subpel_refine(&P, src, w.d_me, w.d_me_sub, P.me_range, (int)g, 1, s2));
        HIPCHK(c, hipEventRecord(c->me_ev[g], s2));
      }
    if ((f + 1) % grp == 0 && f + 1 < n_frames) {   // a full group that is not the last: hand it to the third stream
      if (c->grp_ev.size() <= n_grp) { hipEvent_t e; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->grp_ev.push_back(e); }
      HIPCHK(c, hipEventRecord(c->grp_ev[n_grp], s));
      HIPCHK(c, hipStreamWaitEvent(c->stream3, c->grp_ev[n_grp], 0));
      HIPCHK(c, av1mi_launch_entropy(&P, w.d_cdf, w.d_levels, w.d_blk, w.d_streams, w.d_sym, w.d_combos, w.d_slots, w.d_tile_bytes, w.d_lrc,
                                     w.d_tile_off, nullptr, nullptr, (int)(f + 1 - grp), (int)grp, c->stream3, nullptr, nullptr, nullptr, nullptr));
      n_grp++;
    }
  }
  if (n_grp) HIPCHK(c, hipEventRecord(c->ev[EV_GROUPS_JOINED], c->stream3));
  const int rc = entropy_code(c, n_grp * grp, n_frames);
  return rc ? rc : sse_beside_range_coder(c, src);
}

// The packed bitstream into a buffer for the caller, the final frames into `recon` if asked for, and the report.
// One copy brings the chunk record (frame offsets, symbol counts, overflow flag) to page-locked memory; the host waits for it, then
// fetches exactly the bytes produced.  (Copying a guessed size behind packing without that wait was measured and left out: DESIGN 5d.)
static int download_chunk(av1mi_ctx *c, const Resolved &r, uint32_t n_frames, int frames_on_device, av1mi_buf *out, uint32_t *frame_sizes,
                          void *recon, av1mi_report *report) {
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream, s2 = c->stream2;
  const Av1miChunkRecord &rec = *w.h_record;
  const unsigned long long *foff = reinterpret_cast<const unsigned long long *>(w.h_record + 1);
  hipError_t e1 = hipMemcpyAsync(w.h_record, w.d_record, sizeof(Av1miChunkRecord) + (n_frames + 1) * 8, hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(s);
  if (e1 != hipSuccess) {
    (void)hipStreamSynchronize(s2);
    set_err(c, "fetching the chunk record failed: %s", hipGetErrorString(e1));
    return AV1MI_E_HIP;
  }
  // overflow or a size beyond the buffer end the chunk (the retry reuses the buffers the second stream is still reading, and `recon`
  // may be the caller's memory: it drains first)
  if (rec.overflow || foff[n_frames] > w.out_cap) {
    (void)hipStreamSynchronize(s2);
    if (rec.overflow) set_err(c, "a tile outgrew its %d-byte bitstream slot or its %d-entry symbol stream", P.tile_slot_bytes, P.stream_cap);
    else set_err(c, "internal: packed size exceeds buffer");
    return AV1MI_E_OVERFLOW;
  }
  const size_t total = (size_t)foff[n_frames];
  // the caller's buffer: a page-locked block of the pool (the copy lands in it directly); plain memory + this context's staging
  // buffer only if page-locked memory cannot be had
  uint8_t *host = (uint8_t *)pin_acquire(total ? total : 1), *dst = host;
  if (!host) {
    host = (uint8_t *)malloc(total ? total : 1);
    if (!host) { (void)hipStreamSynchronize(s2); return AV1MI_E_OOM; }
    if (w.h_out_cap < total) {
      w.h_out_cap = 0;
      if (ws_alloc(w, w.h_out, total + (total >> 2) + 4096, true) == hipSuccess) w.h_out_cap = total + (total >> 2) + 4096;
    }
    if (w.h_out && w.h_out_cap >= total) dst = w.h_out;   // (else: straight into the plain block, a staged copy)
    else dst = host;
  }
  e1 = hipMemcpyAsync(dst, w.d_out, total, hipMemcpyDeviceToHost, s);
  hipError_t e2 = hipEventRecord(c->ev[EV_DOWNLOAD_DONE], s);
  if (e2 == hipSuccess) e2 = hipStreamWaitEvent(s, c->ev[EV_CDEF_DONE], 0);  // join: the final reconstruction and the SSE come from the second stream
  if (e1 == hipSuccess && e2 == hipSuccess && recon) {
    const void *fin = w.d_fin;
    if (r.padded) {  // crop to the signalled size, in the caller's tight layout
      e1 = av1mi_launch_pad(w.d_fin, w.d_stage, (int)r.p.width, (int)r.p.height, r.cw, r.ch, P.bit_depth, (int)n_frames, 1, s);
      fin = w.d_stage;
    }
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(recon, fin, caller_bytes(r, n_frames), frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s);
  }
  const unsigned long long *sse = w.h_sse;
  if (e1 == hipSuccess) e1 = hipMemcpyAsync(w.h_sse, w.d_sse, (size_t)n_frames * 24, hipMemcpyDeviceToHost, s);
  // the level search's tables and levels (av1mi_lf_search_result): one more small copy before the wait below.  The levels sit behind the
  // whole workspace's tables, not behind this chunk's: two copies when the chunk is shorter
  const size_t lf_err_bytes = (size_t)n_frames * 3 * AV1MI_LF_CANDS * sizeof(unsigned long long);
  if (e1 == hipSuccess && P.lf_search) e1 = hipMemcpyAsync(w.h_lf, w.d_lf_err, lf_err_bytes, hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && P.lf_search) e1 = hipMemcpyAsync(w.h_lf + lf_err_bytes, w.d_lf_sel, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s);
  // the self-guided fit's errors and records (av1mi_lr_fit_result), likewise
  const size_t fit_n = (size_t)n_frames * 3 * av1mi_lr_unit_rows(P) * av1mi_lr_unit_cols(P);
  if (e1 == hipSuccess && P.lr_fit_code) e1 = hipMemcpyAsync(w.h_fit, w.d_fit, av1mi_lr_fit_result_bytes(fit_n), hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && P.lr_wfit_code) e1 = hipMemcpyAsync(w.h_wfit, w.d_wfit, av1mi_lr_wfit_result_bytes(fit_n), hipMemcpyDeviceToHost, s);   // (av1mi_lr_wiener_fit_result)
  // the bitstream is on the host once EV_DOWNLOAD_DONE has passed: hand it over to the caller's buffer while the second stream finishes
  if (e1 == hipSuccess && e2 == hipSuccess && dst != host) {
    e1 = hipEventSynchronize(c->ev[EV_DOWNLOAD_DONE]);
    if (e1 == hipSuccess) memcpy(host, dst, total);
  }
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(s);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipStreamSynchronize(s2);
    av1mi_free(host);
    set_err(c, "device-to-host copy failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return AV1MI_E_HIP;
  }
  out->data = host; out->size = total;
  c->lf_levels.resize((size_t)n_frames * 4);
  c->lf_errs.assign((size_t)n_frames * 3 * AV1MI_LF_CANDS, 0);
  if (P.lf_search) {
    memcpy(c->lf_errs.data(), w.h_lf, lf_err_bytes);
    memcpy(c->lf_levels.data(), w.h_lf + lf_err_bytes, (size_t)n_frames * 4);
  } else {
    for (uint32_t f = 0; f < n_frames; f++) for (int i = 0; i < 4; i++) c->lf_levels[(size_t)f * 4 + i] = (uint8_t)av1mi_frame_lf_levels(P, (int)f)[i];
  }
  c->fit_units = fit_n; c->fit_plane_units = (uint32_t)(av1mi_lr_unit_rows(P) * av1mi_lr_unit_cols(P));
  c->fit_on = P.lr_fit_code != nullptr;   // (the values stay in h_fit until the context's next chunk)
  c->wfit_on = P.lr_wfit_code != nullptr;
  if (frame_sizes) for (uint32_t f = 0; f < n_frames; f++) frame_sizes[f] = (uint32_t)(foff[f + 1] - foff[f]);
  if (report) {
    memset(report, 0, sizeof(*report));
    report->frames = n_frames; report->bytes = total; report->chunks = 1;
    report->cap_scale = (uint32_t)c->cap_scale; report->gpus_used = 1u << (c->device & 31);
    const double mx = (double)((1 << P.bit_depth) - 1);
    for (int pl = 0; pl < 3; pl++) {
      double t = 0;
      for (uint32_t f = 0; f < n_frames; f++) t += (double)sse[f * 3 + pl];
      report->sse[pl] = t;
      const double npx = (double)n_frames * P.width * P.height / (pl ? 4 : 1);
      report->psnr[pl] = t > 0 ? 10.0 * log10(mx * mx * npx / t) : 99.0;
    }
    report->n_symbols = rec.n_symbols; report->max_tile_symbols = rec.max_tile_symbols;
    (void)hipEventElapsedTime(&report->ms_h2d, c->ev[EV_START], c->ev[EV_SRC_READY]);
    (void)hipEventElapsedTime(&report->ms_recon, c->ev[EV_SRC_READY], c->ev[EV_RECON_DONE]);
    (void)hipEventElapsedTime(&report->ms_cdef, c->ev[EV_CDEF_START], c->ev[EV_CDEF_DONE]);
    (void)hipEventElapsedTime(&report->ms_entropy, c->ev[EV_RECON_DONE], c->ev[EV_ENTROPY_DONE]);
    (void)hipEventElapsedTime(&report->ms_symbolize, c->ev[EV_RECON_DONE], c->ev[EV_SYM_DONE]);
    (void)hipEventElapsedTime(&report->ms_pack, c->ev[EV_ENTROPY_DONE], c->ev[EV_PACK_DONE]);
    (void)hipEventElapsedTime(&report->ms_d2h, c->ev[EV_PACK_DONE], c->ev[EV_DOWNLOAD_DONE]);
    (void)hipEventElapsedTime(&report->ms_total, c->ev[EV_START], c->ev[EV_DOWNLOAD_DONE]);
  }
  return AV1MI_OK;
}

static int run_chunk(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                     av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report);

static int encode_chunk_once(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                             av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report) {
  const int rc = run_chunk(c, params, frames, n_frames, frames_on_device, out, frame_sizes, recon, report);
  if (rc != AV1MI_OK && rc != AV1MI_E_OVERFLOW) {
    // a chunk that broke off may have left uploads from the page-locked copies in flight or undone: let them end, trust none of them
    (void)hipStreamSynchronize(c->stream);
    c->ws.hdr_bytes = 0; c->ws.cdf_qidx = -1; c->ws.params_on_device = 0;
  }
  return rc;
}

static int run_chunk(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                     av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report) {
  out->data = nullptr; out->size = 0;
  c->lf_levels.clear(); c->lf_errs.clear(); c->fit_units = 0; c->fit_plane_units = 0; c->fit_on = false; c->wfit_on = false; c->sym_tiles = 0;
  c->pi_frames = 0;
  Resolved r;
  int rc = resolve(params, &r);
  if (rc) { set_err(c, "invalid parameters"); return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_workspace(c, r, n_frames);
  if (rc) return rc;
  Workspace &w = c->ws;
  c->P = dev_params(r, n_frames, c->cap_scale, w.d_part, w.d_qm, w.d_aq_map, w.d_cdef_err, w.d_cdef_idx, w.d_cdef_sel, w.d_lf_err, w.d_lf_sel,
                     w.d_record, w.d_sym, w.fit.code, w.wfit.code);
  c->part_inter = r.p.partition_search == 2 && c->P.keyint > 1 && n_frames > 1;   // (the chunk goes through schedule_inter)
  const void *d_src = nullptr;
  rc = prepare_chunk(c, r, frames, n_frames, frames_on_device, &d_src);
  if (rc) return rc;
  const Av1miDevParams &P = c->P;
  if (P.keyint > 1 && n_frames > 1) rc = schedule_inter(c, d_src, n_frames);
  else if (P.enable_lr) rc = schedule_all_key_lr(c, d_src, n_frames);
  else rc = schedule_all_key(c, d_src, n_frames);
  if (rc) return rc;
  // packing and the download of the bitstream need nothing from the second stream: they run beside the tail of its work; the join
  // comes before the reconstruction and the SSE are read (download_chunk)
  for (int stage = 0; stage < 2; stage++)
    HIPCHK(c, av1mi_launch_pack(&P, w.d_slots, w.d_tile_bytes, w.d_tile_off, w.d_frame_size, w.d_payload,
                                reinterpret_cast<unsigned long long *>(w.d_record + 1), w.d_hdr, w.d_out, &w.d_record->overflow, stage, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[EV_PACK_DONE], c->stream));
  rc = download_chunk(c, r, n_frames, frames_on_device, out, frame_sizes, recon, report);
  if (rc == AV1MI_OK && P.part_map) { c->pi_keys = c->part_inter; c->pi_frames = n_frames; c->pi_units = (uint32_t)(P.b8_rows * P.b8_cols); c->pi_sbs = (uint32_t)(P.sb_rows * P.sb_cols); }
  return rc;
}

}  // extern "C"
