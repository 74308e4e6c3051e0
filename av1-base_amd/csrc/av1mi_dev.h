// av1mi_dev.h - host/device shared definitions of the MI355X AV1 chunk encoder.
// Product code (never includes anything from oracle/).
#ifndef AV1MI_DEV_H
#define AV1MI_DEV_H
#include <stdint.h>
#include <stddef.h>
#include "lr_geometry.h"
#include "me_rule.h"
#include "tile_weight_rule.h"
#include "wiener_fit_rule.h"   // and lr_fit_rule.h: the counts that size the fits' buffers below
#ifdef __HIPCC__
#define AV1MI_HD __host__ __device__
#else
#define AV1MI_HD
#endif

// Uniform kernel parameters of one chunk (all frames of a chunk share them).
#define AV1MI_QM_4X4 0
#define AV1MI_QM_8X8 16
#define AV1MI_QM_16X16 80
#define AV1MI_QM_32X32 336
#define AV1MI_QM_PLANE 1360   /* entries per plane type */

struct Av1miQmEntry { uint32_t q, recip; };

// What the host needs of a packed chunk before (and beside) its bytes, in one device record the packing kernels fill (its head cleared
// at the start of the chunk) and one copy fetches: this head, then frame_off[n_frames + 1] - the frames' byte offsets in the packed
// output and, last, its total (the packing kernels get `&overflow` and the offsets as the separate arrays they are to them).
struct Av1miChunkRecord {
  unsigned long long n_symbols;   // symbol-stream entries of all tiles of the chunk
  uint32_t max_tile_symbols;      // ... of its longest tile
  int overflow;                   // a tile outgrew its bitstream slot or its symbol stream: nothing was packed
};
static_assert(sizeof(Av1miChunkRecord) == 16, "the frame offsets follow the head, 8-byte aligned");


struct Av1miDevParams {
  int width, height, bit_depth;   // CODED size: the signalled size rounded up to multiples of 8 (the source is edge-extended)
  int true_w, true_h;             // signalled size: what the decoder crops to, clamps references to and restores within
  int mi_rows, mi_cols;     // 4x4 units
  int sb_rows, sb_cols;     // 64x64 superblocks
  int tile_sb;              // tile size in superblocks, both ways: 1, or 2 when the frame has more than 64 superblock rows/columns
  int tile_rows, tile_cols; // tile grid (the last row/column of tiles may be one superblock short)
  int b8_rows, b8_cols;     // 8x8 units (block-info granularity)
  int n_frames;
  int base_q_idx, qctx;
  int dc_q, ac_q;
  uint32_t dc_recip, ac_recip;  // ceil(2^32 / q)
  // quantiser matrices (using_qmatrix): null, or per plane type (luma | chroma) and square transform size the dequantiser
  // step of every coefficient position, {q2 = Round2(q * Quantizer_Matrix[level][plane > 0][pos], 5), ceil(2^32 / q2)};
  // a plane whose level is 15 (flat) holds q itself.  Offsets AV1MI_QM_*; header fields using_qm, qm_y, qm_uv.  (using_qm in front of
  // the pointer, where padding was: the eight bytes went to frame_q below and every other field keeps its offset.)
  int using_qm;
  const Av1miQmEntry *qm_tab;
  int qm_y, qm_uv;
  int min_bs_log2, max_bs_log2;
  // content-driven partition (av1mi_params.partition_search): null, or per frame of the chunk and superblock the split mask
  // partition_kernel wrote (av1mi_node_split below); a node larger than min_bs_log2 and not larger than max_bs_log2 follows it
  const uint32_t *part_map;
  // activity-adaptive quantisation (av1mi_params.cq_level bits 8-10, aq_rule.h): null, or per frame of the chunk and superblock the
  // quantiser index the superblock is coded with, base_q_idx + 4 d (aq_map_kernel).  The reconstruction takes the steps of the index's
  // slot (av1mi_aq_slot below) once per superblock, symbolize codes the index against the tile's CurrentQIndex (read_delta_qindex);
  // everything else a kernel derives from the quantiser - deblocking level, partition threshold, quantiser-matrix level, coefficient
  // q context, range-coder stages - stays with base_q_idx
  const uint8_t *aq_map;
  // the frame term (av1mi_params.cq_level bits 20-22, tpl_rule.h): null, or per frame of the chunk its own base_q_idx q_f
  // (aq_map_kernel, which writes it into the frame's header as well).  aq_map is then always there - q_f + 4 d, or all q_f when no
  // superblock term is on - and its slots are the wide set (av1mi_aq_slot).  What follows q_f: the header's base_q_idx, the coefficient
  // CDFs' q context (normative) and CurrentQIndex at every tile start (symbolize and the range coder), and through the slot the steps,
  // reciprocals, dead zone, dequantiser and quantiser-matrix slice.  What stays with the chunk's base_q_idx, each an encoder's choice
  // and legal in the stream: the deblocking level and the level search's centre, both partition thresholds, the quantiser-matrix
  // level, lr_lambda, the inter-partition penalty and the range coder's stage choice
  const uint8_t *frame_q;
  uint32_t mode_mask;
  int angle_delta;          // 1: directional winners of the luma mode decision are refined over the angle deltas -3 .. +3
  int edge_filter;          // enable_intra_edge_filter
  int cfl;                  // chroma from luma is a candidate (key frames, blocks up to 32x32)
  int tx_search;            // identity transform for sparse intra luma residuals
  int enable_cdef, cdef_y_pri, cdef_y_sec, cdef_uv_pri, cdef_uv_sec, cdef_damping;
  // CDEF strength search (av1mi_params.cdef_search): cdef_search = 0 - one fixed strength set per frame, the
  // fields above (cdef_bits 0); k = 1..4 - cdef_bits = k - 1, 2^cdef_bits pairs per frame from the candidate pool, chosen on the device
  // (the pointers below are null when it is off).  cdef_err: per [frame][superblock] the 16 luma
  // and 8 chroma candidates' squared errors (cdef_search_kernel); cdef_idx: per [frame][superblock] the superblock's index into its frame's
  // set, -1 where no block is coded (cdef_select_kernel; read by CDEF and coded by symbolize); cdef_sel: per frame 8 slots, the set's pair
  // indices p = 8 l + c.  cdef_str_bit[0 / 1]: bit offset of the first strength field in a key / inter frame header
  int cdef_search, cdef_bits;
  int cdef_str_bit[2];
  unsigned long long *cdef_err;
  int8_t *cdef_idx;
  uint8_t *cdef_sel;
  int disable_cdf_update;
  // plane geometry in samples
  int stride_y, stride_c;
  long plane_off_u, plane_off_v;  // sample offsets of U and V inside a frame
  long frame_samples;             // samples per frame
  // per-tile bitstream slot
  int tile_slot_bytes;
  int stream_cap;                 // 32-bit symbol-stream entries per tile (a multiple of RC_BATCH = 16: the range coder reads whole batches)
  // header blob: sequence header OBU, then one slot of `hdr_slot_bytes` per frame holding that frame's OBU_FRAME
  // payload prefix (frame header + alignment); frame_hdr_bytes = its length on key frames, inter_hdr_bytes on
  // inter frames (frames differ only in type and grain_seed)
  int seq_hdr_bytes, frame_hdr_bytes, inter_hdr_bytes, hdr_slot_bytes;
  int tile_size_bytes;
  // inter coding: key frame every `keyint` frames of the chunk (1 = all key frames); motion search range
  int keyint, me_range;
  int subpel;                     // inter frames: 1 = quarter-sample vectors (refined search) + EIGHTTAP filter; 0 = whole-sample vectors, BILINEAR
  int me_presearch;               // inter frames: 1 = the full search runs around the centre a quarter-resolution pre-search found per superblock
  // deblocking filter: loop_filter_level[0..3] (luma vertical edges, luma horizontal, U, V) of key / inter frames and sharpness
  int lf_level[4], lf_level_inter[4], lf_sharpness;
  // level search (av1mi_params.deblock = 2): lf_search = 1 - the levels above are the header's placeholders and
  // decide only whether a frame is deblocked (level [0] is at least 1); the frames' levels are chosen on the device (the pointers are
  // null when it is off).  lf_search_g[0 / 1]: the level the quantiser formula gives key / inter frames, the centre of the candidate
  // pool; lf_err: per [frame][plane] the 16 candidates' squared errors (deblock_search_kernel); lf_sel: per frame the four levels
  // (deblock_decide_kernel; read by deblock_kernel); lf_bit[0 / 1]: bit offset of loop_filter_level[0] in a key / inter frame header
  int lf_search, lf_search_g[2], lf_bit[2];
  unsigned long long *lf_err;
  uint8_t *lf_sel;
  // loop restoration (luma Wiener, 64x64 units): literal bits that code candidate k's coefficients against the
  // reference RefLrWiener (both passes), MSB first in the low `lr_code_len[r][k]` bits
  int enable_lr;                         // the frames' restoration type: 1 = RESTORE_WIENER, 2 = RESTORE_SWITCHABLE (any plane)
  int lr_code_len[4][3];                 // [reference: 0 = Wiener_Taps_Mid, r = candidate r-1][candidate]
  // av1mi_params.enable_lr bits 14 and 15: the unit decisions minimise 16 D + lr_lambda B16 (lr_rate_rule.h); 0 = by
  // the error alone.  The fixed candidates' B16 come from the lengths against reference 0 here and below.  (In what was padding.)
  uint32_t lr_lambda;
  unsigned long long lr_code_bits[4][3];
  // enable_lr = 2: the same for a self-guided unit (lr_sgr_set + both weights against RefSgrXqd; reference 0 = Sgrproj_Xqd_Mid)
  int sgr_code_len[4][3];
  unsigned long long sgr_code_bits[4][3];
  // av1mi_params.enable_lr 3 / 4: U and V are restored as well, with enable_lr's type, in 32x32 units
  // (lr_uv_shift 1); unit choices and sums are then [frame][plane][unit], else [frame][unit].  A chroma Wiener unit codes taps 1
  // and 2 of each pass only (tap 0 is 0): its bit strings, against the plane's RefLrWiener; self-guided units share luma's.
  int lr_chroma;
  // av1mi_params.enable_lr bits 12-13: luma units of 64 << lr_unit_shift samples, chroma units of half that
  int lr_unit_shift;
  int lr_code_len_uv[4][3];
  unsigned long long lr_code_bits_uv[4][3];
  // the self-guided fit (av1mi_params.enable_lr bit 8): null, or per [frame][plane 0..2][unit] the bit string
  // { bits, length } of a self-guided unit, fixed candidates included (lr_fit_kernel.hip); unit choices are then 0 .. 22, 7 + t = set t
  const uint32_t *lr_fit_code;
  // the Wiener fit (av1mi_params.enable_lr bit 10): null, or per [frame][plane 0..2][unit] the bit string
  // { bits 0-31, bits 32-63, length } of a Wiener unit, fixed filters included (lr_wfit_kernel.hip); choice 23 is then the fitted filter
  const uint32_t *lr_wfit_code;
  // packing: null (no counts wanted), or the chunk's record and the [frame][tile] symbol-stream lengths frame_layout_kernel reduces into it
  Av1miChunkRecord *chunk_record;
  const uint32_t *tile_symbols;
};
static_assert(sizeof(Av1miDevParams) == 864, "lr_lambda took padding: the block, a kernel argument, keeps its size");

// ---- adaptive quantisation: the parameter block in device memory is followed by one copy per quantiser slot, equal to it except for
// dc_q, ac_q, their reciprocals and the quantiser-matrix slice.  Slot 0 is the block itself (base_q_idx); slot 1 + 6 + d holds
// base_q_idx + 4 d, d = -6 .. 6 (an index outside 1 .. 255 never occurs in a map: its slot repeats the base).
// With the frame term (frame_q) the set is wide: slot 1 + 16 + j holds base_q_idx + 4 j, j = k_f + d = -16 .. 10 - 28 blocks, five bits.
#define AV1MI_AQ_SLOTS 14
#define AV1MI_FQ_SLOTS 28
AV1MI_HD inline int av1mi_aq_slots(bool wide) { return wide ? AV1MI_FQ_SLOTS : AV1MI_AQ_SLOTS; }
AV1MI_HD inline int av1mi_aq_slot(int qindex, int base_q_idx, bool wide = false) { return (wide ? 17 : 7) + (qindex - base_q_idx) / 4; }
AV1MI_HD inline int av1mi_aq_slot_qindex(int slot, int base_q_idx, bool wide = false) {
  const int q = slot ? base_q_idx + 4 * (slot - (wide ? 17 : 7)) : base_q_idx;
  return q >= 1 && q <= 255 ? q : base_q_idx;
}
// coefficient q context (spec 8.3.2 init_coeff_cdfs): which of the four sets of default coefficient CDFs a frame of this base_q_idx starts from
AV1MI_HD inline int av1mi_q_context(int qidx) { return qidx <= 20 ? 0 : (qidx <= 60 ? 1 : (qidx <= 120 ? 2 : 3)); }

// ---- partition: does the node of size 2^bsl at superblock-local (ox, oy) split?  One rule for every kernel that
// walks blocks (reconstruction, motion search, symbolize).  The syntax forces a split where the node's half point is outside the
// frame (has_rows / has_cols of spec 5.11.4; a leaf may overhang the frame edge by less than half its size); nodes above max_bs_log2
// split, nodes at min_bs_log2 (and 8x8) never do; in between the superblock's split mask decides - bit 0: the 64x64 node, bits
// 1 .. 4: its 32x32 quadrants in Z order, bits 5 .. 20: the sixteen 16x16 nodes in Z order - or, without a mask, the node is a leaf.
AV1MI_HD inline int av1mi_node_split(int width, int height, int min_bs_log2, int max_bs_log2, int have_mask, uint32_t mask,
                                     int sb_x, int sb_y, int ox, int oy, int bsl) {
  const int n = 1 << bsl;
  if (bsl <= 3) return 0;
  if (sb_y + oy + (n >> 1) >= height || sb_x + ox + (n >> 1) >= width) return 1;
  if (bsl <= min_bs_log2) return 0;
  if (bsl > max_bs_log2) return 1;
  if (!have_mask) return 0;
  const int bit = bsl == 6 ? 0 : (bsl == 5 ? 1 + ((oy >> 5) << 1 | (ox >> 5))
                                           : 5 + (((ox >> 4) & 1) | (((oy >> 4) & 1) << 1) | (((ox >> 5) & 1) << 2) | (((oy >> 5) & 1) << 3)));
  return (int)((mask >> bit) & 1u);
}
// log2 size of the leaf whose origin is superblock-local (bx, by), or 0 if (bx, by) is not the origin of a leaf
AV1MI_HD inline int av1mi_leaf_bsl_at(int width, int height, int min_bs_log2, int max_bs_log2, int have_mask, uint32_t mask,
                                      int sb_x, int sb_y, int bx, int by) {
  for (int bsl = 6; bsl >= 3; bsl--) {
    const int n = 1 << bsl;
    const int ox = bx & ~(n - 1), oy = by & ~(n - 1);
    if (!av1mi_node_split(width, height, min_bs_log2, max_bs_log2, have_mask, mask, sb_x, sb_y, ox, oy, bsl)) return (ox == bx && oy == by) ? bsl : 0;
  }
  return 0;
}

// ---- motion search keys (me_kernel.hip -> recon_kernel.hip): me_rule.h has the layouts, av1mi_me_key_decode and the centre code

// frame f of a chunk is a key frame iff f % keyint == 0
AV1MI_HD inline int av1mi_frame_is_inter(const Av1miDevParams &P, int f) { return P.keyint > 1 && (f % P.keyint) != 0; }

// ---- loop restoration (lr_geometry.h): a plane's grid of units at the chunk's unit size, from the signalled size, and the units of one
// frame over its restored planes - the frame stride of the [frame][plane][unit] choices and sums.  The cells - the units of shift 0 - are
// the kernels' work items at every unit size
AV1MI_HD inline int av1mi_lr_cell_rows(const Av1miDevParams &P) { return av1mi_lr_count(P.true_h, 0); }
AV1MI_HD inline int av1mi_lr_cell_cols(const Av1miDevParams &P) { return av1mi_lr_count(P.true_w, 0); }
AV1MI_HD inline int av1mi_lr_unit_rows(const Av1miDevParams &P) { return av1mi_lr_count(P.true_h, P.lr_unit_shift); }
AV1MI_HD inline int av1mi_lr_unit_cols(const Av1miDevParams &P) { return av1mi_lr_count(P.true_w, P.lr_unit_shift); }
AV1MI_HD inline int av1mi_lr_frame_units(const Av1miDevParams &P) { return (P.lr_chroma ? 3 : 1) * av1mi_lr_unit_rows(P) * av1mi_lr_unit_cols(P); }
// the grid of the restoration kernels for `count` frames.  Luma: AV1MI_LR_SLICES waves per cell; chroma: per frame and plane, cell rows x
// pairs of cell columns, AV1MI_LR_SLICES_C waves each (the signalled size is even, so the chroma grid is the luma one)
#define AV1MI_LR_SLICES 7
#define AV1MI_LR_SLICES_C 4
AV1MI_HD inline int av1mi_lr_grid(const Av1miDevParams &P, int count) {
  const int crows = av1mi_lr_cell_rows(P), ccols = av1mi_lr_cell_cols(P);
  return count * crows * ccols * AV1MI_LR_SLICES + (P.lr_chroma ? count * 2 * crows * ((ccols + 1) / 2) * AV1MI_LR_SLICES_C : 0);
}

// the self-guided fit's buffers, all [frame][plane 0..2][unit] whichever planes are restored (lr_fit_kernel.hip)
struct Av1miLrFit {
  long long *sums;            // [16 sets][5]: H00, H01, H11, C0, C1 (lr_fit_rule.h)
  unsigned long long *err;    // [23 candidates]: the exact SSE; ~0 for an absent candidate
  int8_t *rec;                // [4]: choice, set, xqd0, xqd1
  uint32_t *code;             // [2]: bits, length of a self-guided unit's syntax
  uint32_t mask;              // the sets searched (never 0)
  // the buffers from frame `frame0` on, a frame being `upf` units (three planes)
  Av1miLrFit at_frame(int frame0, size_t upf) const {
    const size_t u = (size_t)frame0 * upf;
    return { sums + u * AV1MI_LR_FIT_SETS * 5, err + u * AV1MI_LR_FIT_CANDS, rec + u * 4, code + u * 2, mask };
  }
};
// A chunk's `n` units are one block, contiguous from its head: errors, records - the part the host fetches for av1mi_lr_fit_result -
// then, from a multiple of 8 bytes on, sums and codes
inline size_t av1mi_lr_fit_result_bytes(size_t n) { return n * (AV1MI_LR_FIT_CANDS * 8 + 4); }
inline size_t av1mi_lr_fit_bytes(size_t n) { return av1mi_lr_fit_result_bytes(n) + 8 + n * (AV1MI_LR_FIT_SETS * 5 * 8 + 2 * 4); }
inline Av1miLrFit av1mi_lr_fit_split(void *block, size_t n, uint32_t mask) {
  Av1miLrFit F;
  F.err = reinterpret_cast<unsigned long long *>(block);
  F.rec = reinterpret_cast<int8_t *>(F.err + n * AV1MI_LR_FIT_CANDS);
  F.sums = reinterpret_cast<long long *>(F.rec + ((n * 4 + 7) & ~(size_t)7));
  F.code = reinterpret_cast<uint32_t *>(F.sums + n * AV1MI_LR_FIT_SETS * 5);
  F.mask = mask;
  return F;
}

// the Wiener fit's buffers, likewise [frame][plane 0..2][unit] (lr_wfit_kernel.hip)
struct Av1miLrWfit {
  unsigned long long *err;    // the fitted filter's exact SSE; ~0 if the candidate is absent
  int8_t *rec;                // [8]: final choice 0 .. 23, candidate present, cv0, cv1, cv2, ch0, ch1, ch2
  long long *sums;            // [27] (wiener_fit_rule.h)
  uint32_t *code;             // [3]: bits 0-31, bits 32-63, length of a Wiener unit's syntax
  Av1miLrWfit at_frame(int frame0, size_t upf) const {
    const size_t u = (size_t)frame0 * upf;
    return { err + u, rec + u * 8, sums + u * AV1MI_LR_WFIT_SUMS, code + u * 3 };
  }
};
// likewise one block: errors, records - the part the host fetches for av1mi_lr_wiener_fit_result - sums, codes
inline size_t av1mi_lr_wfit_result_bytes(size_t n) { return n * (8 + 8); }
inline size_t av1mi_lr_wfit_bytes(size_t n) { return av1mi_lr_wfit_result_bytes(n) + n * (AV1MI_LR_WFIT_SUMS * 8 + 3 * 4); }
inline Av1miLrWfit av1mi_lr_wfit_split(void *block, size_t n) {
  Av1miLrWfit F;
  F.err = reinterpret_cast<unsigned long long *>(block);
  F.rec = reinterpret_cast<int8_t *>(F.err + n);
  F.sums = reinterpret_cast<long long *>(F.rec + n * 8);
  F.code = reinterpret_cast<uint32_t *>(F.sums + n * AV1MI_LR_WFIT_SUMS);
  return F;
}

// ---- which symbolize variant owns a tile (entropy_kernel.hip: the kernels decide per tile, the launcher sizes its grids by it)
// Under a content-driven partition (P.part_map, device memory: device code only): does the superblock keep one block size throughout -
// no node between min_bs_log2 and max_bs_log2 splits by its mask?  (Only then does a tile hold exactly two (transform size, plane type)
// classes.)
AV1MI_HD inline bool av1mi_sb_unsplit(const Av1miDevParams &P, int f, int sbr, int sbc) {
  if (!P.part_map || P.min_bs_log2 >= P.max_bs_log2) return true;
  const uint32_t m = P.part_map[((size_t)f * P.sb_rows + sbr) * P.sb_cols + sbc];
  return P.max_bs_log2 >= 6 ? !(m & 1u) : (P.max_bs_log2 == 5 ? !(m & 0x1Eu) : !(m & 0x1FFFE0u));
}
// ... and does the frame edge leave it alone?  A node of the leaf size whose origin lies inside the frame must not be forced to split
// (has_rows / has_cols of av1mi_node_split: a leaf may overhang the edge by less than half its size - the bottom superblock row of a
// 1080-row frame, 56 rows, keeps its four 32x32 leaves; a row of 40 would not).
AV1MI_HD inline bool av1mi_sb_uniform(const Av1miDevParams &P, int f, int sbr, int sbc) {
  if (!av1mi_sb_unsplit(P, f, sbr, sbc)) return false;
  const int L = P.max_bs_log2, n = 1 << L;
  if (L <= 3) return true;
  for (int oy = 0; oy < 64; oy += n)
    for (int ox = 0; ox < 64; ox += n) {
      const int x = sbc * 64 + ox, yy = sbr * 64 + oy;
      if (x < P.width && yy < P.height && (yy + (n >> 1) >= P.height || x + (n >> 1) >= P.width)) return false;
    }
  return true;
}
// The regular variant's tiles: adaptive CDFs and every superblock of the tile (tsb x tsb of them) uniform; all others are the full variant's.
AV1MI_HD inline bool av1mi_tile_is_regular(const Av1miDevParams &P, int f, int tr, int tc, int tsb) {
  if (P.disable_cdf_update) return false;
  for (int si = 0; si < tsb * tsb; si++) {
    const int sbr = tr * tsb + si / tsb, sbc = tc * tsb + si % tsb;
    if (sbr < P.sb_rows && sbc < P.sb_cols && !av1mi_sb_uniform(P, f, sbr, sbc)) return false;
  }
  return true;
}
// Without a partition map ownership is geometry, the same in every frame, and a superblock that is not uniform lies in the last
// superblock row or column: the full variant's tiles are among a frame's edge tiles - its last tile row, then the last tile column
// above it, tile_cols + tile_rows - 1 in all.  Edge tile e of a frame:
AV1MI_HD inline int av1mi_edge_tiles(const Av1miDevParams &P) { return P.tile_cols + P.tile_rows - 1; }
AV1MI_HD inline int av1mi_edge_tile(const Av1miDevParams &P, int e) {
  return e < P.tile_cols ? (P.tile_rows - 1) * P.tile_cols + e : (e - P.tile_cols) * P.tile_cols + P.tile_cols - 1;
}

// Per 8x8-unit block info written by the recon kernel, read by entropy + CDEF kernels.
// Only the entry at a block's top-left 8x8 unit carries eobs; mode/skip are replicated over the
// block so neighbour-context lookups are direct.
struct Av1miBlkInfo {
  uint8_t ymode;
  uint8_t skip;
  uint8_t bsl;      // log2 block size in pixels (3..6)
  uint8_t is_inter; // inter frames: 1 = predicted from LAST_FRAME with `mv`
  uint16_t eob[3];
  int16_t mv_row, mv_col;  // 1/8 luma samples
  uint16_t angle;   // bits 0-2: angle delta + 3 of a directional intra mode (3 = none), luma and chroma alike; bit 3: luma IDTX;
                    // bits 4-9 / 10-15: chroma-from-luma alpha U / V (6-bit two's complement; both zero = not chroma from luma)
};
static_assert(sizeof(Av1miBlkInfo) == 16, "block info is one 16-byte record");

#define AV1MI_SB_LEVELS 6144  // int16 levels per superblock: 64*64 + 2*32*32
// Offset of a block's levels inside its superblock's 6144: blocks are stored in Morton (Z) order of their origin's
// 8x8 unit - a block of n x n samples at a quadtree-aligned origin covers (n/8)^2 consecutive Morton indices, so its
// n*n levels are contiguous and blocks of any mix of sizes never overlap.  Luma 64 levels per unit, then U and V with
// 16 per unit.  (bx, by): luma sample position of the block inside the superblock.
AV1MI_HD inline int av1mi_morton8(int ux, int uy) {
  return (ux & 1) | ((uy & 1) << 1) | ((ux & 2) << 1) | ((uy & 2) << 2) | ((ux & 4) << 2) | ((uy & 4) << 3);
}
AV1MI_HD inline int av1mi_levels_off(int plane, int bx, int by) {
  const int m = av1mi_morton8(bx >> 3, by >> 3);
  return plane == 0 ? m * 64 : 4096 + (plane - 1) * 1024 + m * 16;
}

// Default-CDF blob layout (uint16 inverted CDFs, each row n+1 entries: n-1 values, 0, counter)
// for one q context; offsets in uint16 units.  Mirrors the per-tile adaptive state.
struct Av1miCdfLayout {
  enum {
    PARTITION = 0,                         // [16][11]  (8x8 .. 64x64: no 128x128 superblocks)
    KF_Y_MODE = PARTITION + 16 * 11,       // [5][5][14]
    UV_MODE = KF_Y_MODE + 25 * 14,         // [2][13][15]
    ANGLE_DELTA = UV_MODE + 26 * 15,       // [8][8]
    SKIP = ANGLE_DELTA + 64,               // [3][3]
    TX_SET1 = SKIP + 9,                    // [2][13][8]
    TX_SET2 = TX_SET1 + 26 * 8,            // [3][13][6]
    TXB_SKIP = TX_SET2 + 39 * 6,           // [5][13][3]
    EOB16 = TXB_SKIP + 65 * 3,             // [2][2][6]
    EOB32 = EOB16 + 4 * 6,                 // [2][2][7]
    EOB64 = EOB32 + 4 * 7,
    EOB128 = EOB64 + 4 * 8,
    EOB256 = EOB128 + 4 * 9,
    EOB512 = EOB256 + 4 * 10,
    EOB1024 = EOB512 + 4 * 11,
    EOB_EXTRA = EOB1024 + 4 * 12,          // [5][2][9][3]
    DC_SIGN = EOB_EXTRA + 90 * 3,          // [2][3][3]
    COEFF_BASE_EOB = DC_SIGN + 6 * 3,      // [5][2][4][4]
    USE_WIENER = COEFF_BASE_EOB + 40 * 4,  // [3]
    RESTORE_SW = USE_WIENER + 3,           // [4] restoration_type of RESTORE_SWITCHABLE frames: NONE, WIENER, SGRPROJ
    CFL_SIGN = RESTORE_SW + 4,             // [9]
    CFL_ALPHA = CFL_SIGN + 9,              // [6][17]
    DELTA_Q = CFL_ALPHA + 6 * 17,          // [5] delta_q_abs (adaptive quantisation)
    COEFF_BASE = DELTA_Q + 5,              // [5][2][42][5]
    COEFF_BR = COEFF_BASE + 420 * 5,       // [5][2][21][5]
    INTRA_TOTAL = COEFF_BR + 210 * 5,      // everything a key frame needs
    // inter frames
    INTER_BASE = INTRA_TOTAL,
    IF_Y_MODE = INTER_BASE,                // [4][14]
    IS_INTER = IF_Y_MODE + 4 * 14,         // [4][3]
    NEWMV = IS_INTER + 4 * 3,              // [6][3]
    GLOBALMV = NEWMV + 6 * 3,              // [2][3]
    REFMV = GLOBALMV + 2 * 3,              // [6][3]
    DRL = REFMV + 6 * 3,                   // [3][3]
    SINGLE_REF = DRL + 3 * 3,              // [6 p1..p6][3 ctx][3]
    INTER_TX1 = SINGLE_REF + 18 * 3,       // [2][17]
    INTER_TX2 = INTER_TX1 + 2 * 17,        // [13]
    INTER_TX3 = INTER_TX2 + 13,            // [4][3]
    MV_JOINT = INTER_TX3 + 4 * 3,          // [5]
    MV_COMP = MV_JOINT + 5,                // [2] x { class[12], class0_fp[2][5], fp[5], sign[3], class0_hp[3], hp[3], class0[3], bits[10][3] }
    MVC_CLASS = 0, MVC_CLASS0_FP = 12, MVC_FP = 22, MVC_SIGN = 27, MVC_CLASS0_HP = 30, MVC_HP = 33, MVC_CLASS0 = 36, MVC_BITS = 39,
    MVC_SIZE = 69,
    TOTAL = MV_COMP + 2 * MVC_SIZE
  };
};

// The wide rows as the regular symbolize variants keep them (entropy_kernel.hip): a regular tile has one luma and one chroma transform
// size, so the tables the full layout keeps per size - a third of the wide rows - shrink to one slice per plane type: 3.2 instead of
// 4.9 KB.  PARTITION .. SKIP keep their offsets.  The image depends on the blob and the leaf size alone, so the host builds it once
// where it makes the blob (av1mi_cdf_compact_build) and uploads it behind the blob, at AT; a tile's wave copies it in 16-byte pieces.
struct Av1miCdfCompact {
  typedef Av1miCdfLayout CL;
  enum {
    LEAD = CL::TX_SET1,
    TXSET = LEAD,                        // the luma size's slice of TX_SET1 ([13][8]) or TX_SET2 ([13][6]), if it has one
    TXB_SKIP = TXSET + 13 * 8,           // [2 plane types][13][3]
    EOB = TXB_SKIP + 2 * 13 * 3,         // [2][12]: the row (context 0) of the plane type's size
    EOB_EXTRA = EOB + 2 * 12,            // [2][9][3]
    DC_SIGN = EOB_EXTRA + 2 * 9 * 3,     // [2][3][3] as in the full layout
    COEFF_BASE_EOB = DC_SIGN + 18,       // [2][4][4]
    USE_WIENER = COEFF_BASE_EOB + 2 * 16, RESTORE_SW = USE_WIENER + 3, CFL_SIGN = RESTORE_SW + 4, CFL_ALPHA = CFL_SIGN + 9,
    DELTA_Q = CFL_ALPHA + 6 * 17,
    TOTAL = DELTA_Q + 5,
    WORDS = (TOTAL + 18 + 7) & ~7,       // + 18: whole-row reads by 17 lanes may run past the last row; whole 16-byte pieces
    AT = (CL::TOTAL + 7) & ~7,           // offset of the image in the uploaded blob (16-byte aligned)
    BLOB_WORDS = AT + WORDS
  };
};
static_assert(Av1miCdfLayout::COEFF_BASE - Av1miCdfLayout::USE_WIENER == Av1miCdfCompact::TOTAL - Av1miCdfCompact::USE_WIENER, "the trailing tables are copied as one piece");
// the image (WORDS entries) of the blob `cdf` for leaves of 2^max_bs_log2 samples
AV1MI_HD inline void av1mi_cdf_compact_build(const uint16_t *cdf, int max_bs_log2, uint16_t *w) {
  typedef Av1miCdfLayout CL;
  typedef Av1miCdfCompact CC;
  const int l2y = max_bs_log2 > 6 ? 6 : max_bs_log2, l2c = l2y - 1 > 5 ? 5 : l2y - 1;
  for (int i = 0; i < CC::WORDS; i++) w[i] = 0;
  for (int i = 0; i < CC::LEAD; i++) w[i] = cdf[i];
  if (l2y <= 3) for (int i = 0; i < 13 * 8; i++) w[CC::TXSET + i] = cdf[CL::TX_SET1 + (l2y - 2) * 13 * 8 + i];
  else if (l2y == 4) for (int i = 0; i < 13 * 6; i++) w[CC::TXSET + i] = cdf[CL::TX_SET2 + (l2y - 2) * 13 * 6 + i];
  for (int p = 0; p < 2; p++) {
    const int l2 = p ? l2c : l2y, txs = l2 - 2, bwl = l2 > 5 ? 5 : l2, msz = 2 * bwl - 4, nsy = 5 + msz;
    const int eoff = CL::EOB16 + 4 * (msz * 6 + (msz * (msz - 1)) / 2) + (p * 2 + 0) * (nsy + 1);
    for (int k = 0; k < 39; k++) w[CC::TXB_SKIP + p * 39 + k] = cdf[CL::TXB_SKIP + txs * 39 + k];
    for (int k = 0; k <= nsy; k++) w[CC::EOB + p * 12 + k] = cdf[eoff + k];
    for (int k = 0; k < 27; k++) w[CC::EOB_EXTRA + p * 27 + k] = cdf[CL::EOB_EXTRA + (txs * 2 + p) * 27 + k];
    for (int k = 0; k < 16; k++) w[CC::COEFF_BASE_EOB + p * 16 + k] = cdf[CL::COEFF_BASE_EOB + (txs * 2 + p) * 16 + k];
  }
  for (int i = 0; i < 18; i++) w[CC::DC_SIGN + i] = cdf[CL::DC_SIGN + i];
  for (int i = 0; i < CC::TOTAL - CC::USE_WIENER; i++) w[CC::USE_WIENER + i] = cdf[CL::USE_WIENER + i];
}

#endif
