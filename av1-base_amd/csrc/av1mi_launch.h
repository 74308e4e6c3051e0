// av1mi_launch.h - the kernel launchers: the one declaration of every `av1mi_launch_*`.
// av1mi_host.cpp calls them through this header, and every file that defines one includes it (the four reconstruction translation units
// through recon_kernel.hip): the launchers have C linkage, which carries no types, so only the compiler seeing declaration and
// definition together ("conflicting types") keeps a caller and a definition from drifting apart.
//
// Frames of a chunk.  A launcher that can run on part of a chunk takes the chunk-wide arrays and `(frame0, count)` - frames
// [frame0, frame0 + count) of the chunk P describes.  The search kernels and the entropy coder index the chunk themselves; reconstruction,
// deblocking, CDEF and restoration kernels see a launch's frames only: their launchers (and no one else) advance the arrays to frame0 and
// hand the kernels av1mi_frame_range's parameters.  Every other launcher runs on all P->n_frames frames.
// Blocks.  A pass whose buffers are one allocation takes a struct of pointers into it: the restoration fits' (av1mi_dev.h) and the
// film-grain passes' below, with their split functions, byte sizes and fetched heads.
#ifndef AV1MI_LAUNCH_H
#define AV1MI_LAUNCH_H
#include <hip/hip_runtime.h>
#include "av1mi_dev.h"
#include "../../include/av1mi.h"

// The parameters of a launch over frames [frame0, frame0 + count): n_frames is the launch's, and every per-frame map the kernels index
// from the launch's first frame on starts there - a kernel that is given a range indexes these maps relative to the launch, whether
// or not it reads them.  (A new per-frame map gets its line here.)
inline Av1miDevParams av1mi_frame_range(const Av1miDevParams &P, int frame0, int count) {
  Av1miDevParams R = P;
  const size_t sb0 = (size_t)frame0 * P.sb_rows * P.sb_cols;
  R.n_frames = count;
  if (R.part_map) R.part_map += sb0;
  if (R.aq_map) R.aq_map += sb0;
  if (R.frame_q) R.frame_q += frame0;
  if (R.cdef_idx) R.cdef_idx += sb0;
  if (R.cdef_sel) R.cdef_sel += (size_t)frame0 * 8;
  if (R.lf_err) R.lf_err += (size_t)frame0 * 48;
  if (R.lf_sel) R.lf_sel += (size_t)frame0 * 4;
  return R;
}
// frame f of a chunk-wide array of frames at the coded size (8- or 16-bit samples)
inline const void *av1mi_frame_at(const Av1miDevParams &P, const void *frames, int f) {
  return (const uint8_t *)frames + (size_t)f * P.frame_samples * (P.bit_depth > 8 ? 2 : 1);
}
inline void *av1mi_frame_at(const Av1miDevParams &P, void *frames, int f) { return const_cast<void *>(av1mi_frame_at(P, (const void *)frames, f)); }
// deblocking levels of frame f, by its kind (level [0] zero: the frame is not deblocked - the launcher's and its caller's one rule)
inline const int *av1mi_frame_lf_levels(const Av1miDevParams &P, int f) { return av1mi_frame_is_inter(P, f) ? P.lf_level_inter : P.lf_level; }

// The two blocks of the film-grain passes, described as the restoration fits' are (av1mi_lr_fit_split): one allocation each, a struct of
// pointers into it, its bytes, and the head the host fetches in one copy - a split of the page-locked mirror reads that.
// The estimate's block (fg_kernel.hip), for n records - the pointers at bytes 0, 32, 128, 160 and behind the parts:
#define AV1MI_FG_PARTS 64
struct Av1miFgBlock {
  uint8_t *table;     // the 24 values [plane][bin], clamped to the ceilings
  uint32_t *counts;   // the bins' 24 block counts
  uint8_t *quart;     // the 24 quartiles before the fill and the clamp, 0 for a bin without blocks (fg_ar_kernel.hip's flatness)
  uint32_t *parts;    // scratch: the histograms' parts, AV1MI_FG_PARTS x 24 x 256 counters (16-byte aligned)
  uint32_t *blocks;   // per [frame][16x16 block of the signalled size] the record { bin, v_y, v_u, v_v }, all written (16-byte aligned)
};
inline size_t av1mi_fg_result_bytes() { return 128; }   // table and counts
inline size_t av1mi_fg_bytes(size_t n) { return 160 + ((size_t)AV1MI_FG_PARTS * 24 * 256 + (n ? n : 1)) * sizeof(uint32_t); }
inline Av1miFgBlock av1mi_fg_split(void *block) {
  uint8_t *b = reinterpret_cast<uint8_t *>(block);
  uint32_t *parts = reinterpret_cast<uint32_t *>(b + 160);
  return { b, reinterpret_cast<uint32_t *>(b + 32), b + 128, parts, parts + (size_t)AV1MI_FG_PARTS * 24 * 256 };
}
// The fit's block (fg_ar_kernel.hip), 16-byte aligned: the result at its head - the pointers at bytes 0, 80, 104, 128, 140 and 152 - and
// the workgroups' parts behind it
#define AV1MI_FGAR_MAX_GROUPS 1024
struct Av1miFgArBlock {
  int8_t *coeffs;       // [plane][25]
  uint8_t *table;       // the 24 values scaled by the gains: what the headers carry
  uint8_t *sigma;       // the 24 values unscaled: the estimate's table
  uint32_t *gain;       // [plane], 256 = 1
  uint32_t *flat;       // [plane]: the flat blocks
  long long *sums;      // [plane][46]
  long long *parts;     // [workgroup][plane][47]: the sums and the flat blocks of up to AV1MI_FGAR_MAX_GROUPS workgroups
};
inline size_t av1mi_fgar_result_bytes() { return 1280; }
inline size_t av1mi_fgar_bytes() { return av1mi_fgar_result_bytes() + (size_t)AV1MI_FGAR_MAX_GROUPS * 3 * 47 * 8; }
inline Av1miFgArBlock av1mi_fgar_split(void *block) {
  uint8_t *b = reinterpret_cast<uint8_t *>(block);
  uint32_t *gain = reinterpret_cast<uint32_t *>(b + 128);
  return { reinterpret_cast<int8_t *>(b), b + 80, b + 104, gain, gain + 3, reinterpret_cast<long long *>(b + 152),
           reinterpret_cast<long long *>(b + av1mi_fgar_result_bytes()) };
}
// where make_frame_header left the placeholders the passes overwrite in every frame's header slot: the first luma point (fg_bit) and the
// first luma coefficient (fg_ar_bit) of a key and of an inter frame's header; all 0 without a header blob
struct Av1miFgBits { int fg_key, fg_inter, ar_key, ar_inter; };

// The frame term's block (tpl_rule.h "frame"; tpl_frame_kernel, aq_map_kernel), for n frames, 8-byte aligned: the small results per
// frame in one allocation, which the host fetches in one copy
struct Av1miFqBlock {
  unsigned long long *intra_sum;     // OF = sum I over the frame's blocks
  unsigned long long *dep_sum;       // PF = sum (I + A)
  unsigned long long *sb_beta_sum;   // the sum of beta over the frame's superblocks (Mb_f comes from it)
  uint16_t *beta;                    // betaF
  uint8_t *frame_q;                  // q_f, the frame's base_q_idx (aq_map_kernel)
};
inline size_t av1mi_fq_bytes(size_t n) { return n * 27; }
inline Av1miFqBlock av1mi_fq_split(void *block, size_t n) {
  unsigned long long *q = reinterpret_cast<unsigned long long *>(block);
  uint16_t *b = reinterpret_cast<uint16_t *>(q + 3 * n);
  return { q, q + n, q + 2 * n, b, reinterpret_cast<uint8_t *>(b + n) };
}
// What aq_map_kernel takes of the frame term: strength 0 = off, nothing else is read.  hdr_blob: null, or the chunk's header blob, whose
// frame headers receive q_f in the eight bits of base_q_idx at q_bit[key / inter] (make_frame_header's offsets; not byte-aligned)
struct Av1miFqMap {
  int strength;
  int q_bit[2];
  Av1miFqBlock fq;
  uint8_t *hdr_blob;
};

// What the quality pass (quality_kernel.hip, ssim_rule.h) compares: two chunks of one layout, given explicitly - a frame every
// frame_samples samples, and per plane where it starts in the frame, its row stride (all in samples) and its h x w at the signalled size.
// The callers' tight layout and the encoder's buffers at the coded size are the two uses.  map_at: where a plane's windows start in a
// frame's part of the window map, map_frame the windows of a frame over its three planes
struct Av1miQualityGeom {
  size_t frame_samples;
  size_t off[3];
  int stride[3], w[3], h[3];
  uint32_t map_at[3], map_frame;
  int bit_depth;
};
// a plane's windows (ssim_rule.h: av1mi_ssim_windows both ways)
inline uint32_t av1mi_quality_windows(const Av1miQualityGeom &G, int pl) {
  const int ny = G.h[pl] >= 8 ? (G.h[pl] - 8) / 4 + 1 : 0, nx = G.w[pl] >= 8 ? (G.w[pl] - 8) / 4 + 1 : 0;
  return (uint32_t)ny * (uint32_t)nx;
}
// planar 4:2:0 frames stored at cw x ch with the signalled w x h inside them: cw x ch = w x h is the callers' tight layout
inline Av1miQualityGeom av1mi_quality_geom(int w, int h, int cw, int ch, int bit_depth) {
  Av1miQualityGeom G = {};
  G.frame_samples = (size_t)cw * ch * 3 / 2;
  G.bit_depth = bit_depth;
  for (int pl = 0; pl < 3; pl++) {
    G.off[pl] = pl == 0 ? 0 : (size_t)cw * ch + (pl == 2 ? (size_t)(cw / 2) * (ch / 2) : 0);
    G.stride[pl] = pl ? cw / 2 : cw;
    G.w[pl] = pl ? (w + 1) / 2 : w;
    G.h[pl] = pl ? (h + 1) / 2 : h;
    G.map_at[pl] = G.map_frame;
    G.map_frame += av1mi_quality_windows(G, pl);
  }
  return G;
}

// The film-grain synthesis' block (fg_synth_kernel.hip, fg_synth_rule.h), for n frames of frame_blocks = stripes x blocks 32x32 luma
// blocks each, 16-byte aligned: the parameter set at its head (byte 0) and the three scaling functions (byte 256), then from byte 1024 the
// frames' templates (AV1MI_FGS_TEMPLATE_N = 9330 samples each) and their blocks' values
struct Av1miFgsBlock {
  av1mi_grain_params *g;   // what both kernels read: the caller's, uploaded, or av1mi_launch_fg_synth_params'
  uint8_t *lut;            // [plane][256]
  int16_t *templates;      // [frame][9330]: LumaGrain, CbGrain, CrGrain
  uint8_t *offs;           // [frame][stripe][block]
};
inline size_t av1mi_fgs_bytes(size_t n, size_t frame_blocks) { return 1024 + n * (9330 * sizeof(int16_t) + frame_blocks); }
inline Av1miFgsBlock av1mi_fgs_split(void *block, size_t n) {
  uint8_t *b = reinterpret_cast<uint8_t *>(block);
  return { reinterpret_cast<av1mi_grain_params *>(b), b + 256, reinterpret_cast<int16_t *>(b + 1024), b + 1024 + n * 9330 * sizeof(int16_t) };
}

extern "C" {
// ---- whole chunk (or call): all P->n_frames frames
// the film-grain synthesis (fg_synth_kernel.hip, fg_synth_rule.h), launches on one stream, all reading the parameter set at B.g.
// _params: B.g = what the encoder's frame headers carry with film_grain = N (fg_synth_rule.h: av1mi_fgs_header_params) - table: null for
// the fixed table, else the 24 values in device memory (av1mi_launch_film_grain's, or with a lag av1mi_launch_fg_ar's scaled ones);
// coeffs: null without a lag, else the fit's [plane][25].  A caller with a set of its own copies it to B.g instead.
// _templates: the templates, block values and scaling functions of n_frames frames of w x h luma (both even) into B: seeds null - frame
// f's grain_seed by the encoder's rule from first_frame - or n_frames seeds in device memory.
// _apply: `in`, laid out as Gin says, with its grain into `out`, another block, laid out as Gout says - each the callers' tight layout
// or the encoder's coded size, as the quality pass, of one signalled size; every sample of that size is written, a plane without a scaling
// function copied
hipError_t av1mi_launch_fg_synth_params(int N, int estimate, int lag, const uint8_t *table, const int8_t *coeffs, Av1miFgsBlock B, hipStream_t stream);
hipError_t av1mi_launch_fg_synth_templates(int bit_depth, int w, int h, int n_frames, const uint16_t *seeds, uint32_t first_frame, Av1miFgsBlock B,
                                           hipStream_t stream);
hipError_t av1mi_launch_fg_synth_apply(const Av1miQualityGeom *Gin, const Av1miQualityGeom *Gout, const void *in, void *out, int n_frames,
                                       Av1miFgsBlock B, hipStream_t stream);
// split masks of every superblock (partition_kernel)
hipError_t av1mi_launch_partition(const Av1miDevParams *P, const void *frames, uint32_t *part, hipStream_t stream);
// quantiser index of every superblock (aq_activity_kernel, aq_map_kernel): act and qmap are [frame][superblock].  tpl_strength != 0: the
// temporal term on top (tpl_rule.h) - beta [frame][superblock] and beta_sum, the chunk's sum of it, as av1mi_launch_tpl on the same
// stream before has left them; either strength may be 0, not both - unless the frame term is on.  fq: null, or the frame term
// (fq->strength != 0, behind av1mi_launch_tpl_frames on the same stream): every frame's q_f into fq->fq.frame_q and into its header, the
// map q_f + 4 d with the temporal term against the frame's own mean, or all q_f when both superblock strengths are 0
hipError_t av1mi_launch_aq(const Av1miDevParams *P, const void *frames, uint16_t *act, uint8_t *qmap, int strength, const uint16_t *beta,
                           const unsigned long long *beta_sum, int tpl_strength, const Av1miFqMap *fq, hipStream_t stream);
// the frame term's sums (tpl_frame_kernel), behind av1mi_launch_tpl on the same stream: OF, PF, betaF and the sum of beta of every frame
hipError_t av1mi_launch_tpl_frames(const Av1miDevParams *P, const uint32_t *intra, const unsigned long long *flow, const uint16_t *beta,
                                   Av1miFqBlock fq, hipStream_t stream);
// the temporal-dependency analysis (tpl_kernel.hip, tpl_rule.h) of the chunk's source at the coded size, range P->me_range: per
// [frame][16x16 block] the intra cost, the inter cost, the search's node key (all-ones on key frames) - all written - and the flow, added
// into `flow`; per [frame][superblock] beta.  flow: av1mi_tpl_flow_entries entries, zeroed by the caller - the last one receives the
// chunk's sum of beta.  `frames` must be a 16-byte aligned device pointer (anything else is refused); it is only read
hipError_t av1mi_launch_tpl(const Av1miDevParams *P, const void *frames, uint32_t *intra, uint32_t *inter, uint32_t *key, unsigned long long *flow,
                            uint16_t *beta, hipStream_t stream);
// the film-grain estimate (fg_kernel.hip, fg_rule.h) of the chunk's source: `frames` at the coded size, of which the whole 16x16 blocks of
// the signalled size are read; a 16-byte aligned device pointer, only read.  fg: the estimate's block, split.  The table is clamped to
// ceil_y / ceil_c.  hdr_blob: null, or the chunk's header blob, whose frame headers receive the values at bits.fg_key / bits.fg_inter
hipError_t av1mi_launch_film_grain(const Av1miDevParams *P, const void *frames, Av1miFgBlock fg, int ceil_y, int ceil_c, uint8_t *hdr_blob,
                                   Av1miFgBits bits, hipStream_t stream);
// the grain's autoregressive fit at lag 1 .. 3 (fg_ar_kernel.hip, fg_ar_rule.h) on the same frames, behind av1mi_launch_film_grain on the
// same stream: fg as that launch left it.  ar: the fit's block, split.  hdr_blob: null, or the chunk's header blob, whose frame headers
// receive the scaled values at bits.fg_* and the coefficient bytes at bits.ar_*
hipError_t av1mi_launch_fg_ar(const Av1miDevParams *P, const void *frames, Av1miFgBlock fg, int lag, Av1miFgArBlock ar, uint8_t *hdr_blob,
                              Av1miFgBits bits, hipStream_t stream);
// the source denoised by the film-grain table (fg_denoise_kernel.hip, fg_denoise_rule.h), out of place: `frames` as the caller gave them,
// tight at the signalled size P->true_w x P->true_h, only read; `out` the same frames filtered, at the coded size, samples outside the
// signalled picture replicating the denoised edge; table: the 24 values [plane][bin] in device memory (av1mi_launch_film_grain's, on the
// same stream before).  Both frame pointers must be 16-byte aligned device pointers and different blocks.  span = 1 or 2: with the
// temporal term over so many neighbours each way, by the keys mv[(frame * 4 + slot) * blocks + block] (fg_denoise_rule.h) at range
// P->me_range - av1mi_launch_fg_denoise_search's on the same stream before, or the caller's; span = 0: the spatial filter, mv is not read
hipError_t av1mi_launch_fg_denoise(const Av1miDevParams *P, const void *frames, void *out, const uint8_t *table, const uint32_t *mv, int span,
                                   hipStream_t stream);
// the temporal term's search: `coded`, the undenoised frames at the coded size (a 16-byte aligned device pointer, only read; it may be the
// block the filter launch behind it writes), every frame against its neighbours within `span` at range P->me_range; mv: all its
// P->n_frames * 4 * blocks keys written, all-ones for a neighbour that does not exist
hipError_t av1mi_launch_fg_denoise_search(const Av1miDevParams *P, const void *coded, uint32_t *mv, int span, hipStream_t stream);
// the key frames' temporal filter (tf_kernel.hip, tf_rule.h), in place in `frames` at the coded size: every key frame of the chunk is
// replaced by its filter over up to tf_frames followers at tf_strength, range P->me_range, and re-extended past the signalled size.
// `frames` must be a 16-byte aligned device pointer (both callers pass an allocation of their own; anything else is refused).
// mv: the search's node keys [key frame][tf_frames][16x16 block], all written (all-ones for a follower that does not exist)
hipError_t av1mi_launch_temporal_filter(const Av1miDevParams *P, void *frames, uint32_t *mv, int tf_frames, int tf_strength, hipStream_t stream);
// quarter-resolution luma of all frames
hipError_t av1mi_launch_quarter_luma(const Av1miDevParams *P, const void *frames, uint16_t *quarter, hipStream_t stream);
// `frames` / `prev0` must be 16-byte aligned device pointers (checked by the caller); sad[] zeroed by the caller
hipError_t av1mi_launch_luma_sad(const Av1miDevParams *P, const void *frames, const void *prev0, unsigned long long *sad, hipStream_t stream);
// n_frames frames of w x h edge-extended to cw x ch, or with `crop` frames of cw x ch cut back to w x h
hipError_t av1mi_launch_pad(const void *in, void *out, int w, int h, int cw, int ch, int bit_depth, int n_frames, int crop, hipStream_t stream);
// squared error of a against b into sse[frame][plane] (added)
hipError_t av1mi_launch_sse(const Av1miDevParams *P, const void *a, const void *b, unsigned long long *sse, hipStream_t stream);
// the quality pass (quality_kernel.hip, ssim_rule.h): n_frames frames of `a`, the reference, against `b`, both laid out as G says.
// sums[(frame * 3 + plane) * 2 + 0 / 1]: the plane's squared error and its sum of window values (a two's-complement int64), both ADDED -
// zeroed by the caller.  map: null, or per frame G->map_frame window values, every one written
hipError_t av1mi_launch_quality(const Av1miQualityGeom *G, const void *a, const void *b, int n_frames, unsigned long long *sums, int32_t *map,
                                hipStream_t stream);
// stage 0: the frames' layout, sizes and the chunk record; stage 1: headers and tiles into `out`
hipError_t av1mi_launch_pack(const Av1miDevParams *P, const uint8_t *slots, const uint32_t *tile_bytes, uint32_t *tile_off,
                             uint32_t *frame_size, uint32_t *payload_size, unsigned long long *frame_off, const uint8_t *hdr_blob,
                             uint8_t *out, int *overflow, int stage, hipStream_t stream);

// ---- frames [frame0, frame0 + count) of the chunk; every array is chunk-wide
// search centres of the frames (key frames are skipped)
hipError_t av1mi_launch_presearch(const Av1miDevParams *P, const uint16_t *quarter, uint32_t *centre, int frame0, int count, hipStream_t stream);
// best[] (n_frames x 8x8 units) must be filled with 0xFF bytes before the launch.  Every inter frame is searched against the source frame
// before it.  me_range must be 8 or 16.  acc64: block_log2 = 6 - the zeroed [frame][superblock][candidate] table, else null.
// centre: pre-search centre codes [frame][superblock], or null.
hipError_t av1mi_launch_motion_search(const Av1miDevParams *P, const void *frames, unsigned long long *best, int me_range, int frame0,
                                      int count, uint32_t *acc64, const uint32_t *centre, hipStream_t stream);
// partition_search = 2, instead of av1mi_launch_motion_search: the search in node mode - every node of the partition tree keeps its best
// candidate in `nodes`, the [frame][level][node] tables of part_inter_rule.h filled with 0xFF bytes - then the frames' partition decided
// from those costs: the masks into `part` ([frame][superblock]), the leaves' keys into `best`.  acc64, centre as above.
hipError_t av1mi_launch_inter_partition(const Av1miDevParams *P, const void *frames, unsigned long long *best, int me_range, int frame0, int count,
                                        uint32_t *acc64, const uint32_t *centre, uint32_t *nodes, uint32_t *part, hipStream_t stream);
// Refines the frames' vectors: `best` = the full search's keys (av1mi_launch_motion_search on the same stream before), `refined` = same
// layout, what the reconstruction reads with subpel = 1.
hipError_t av1mi_launch_subpel_refine(const Av1miDevParams *P, const void *frames, const unsigned long long *best, unsigned long long *refined,
                                      int me_range, int frame0, int count, hipStream_t stream);
// One translation unit per (largest leaf, sample type): recon_kernel.hip, recon8_kernel.hip, recon64_kernel.hip, recon64_8_kernel.hip;
// callers go through av1mi_launch_recon below.
// frame0 a key frame: `count` key frames in one launch (fin and me_best are not read).  frame0 an inter frame: that ONE frame (count
// must be 1), predicted from frame frame0 - 1 of `fin`, the final frames, with its keys in `me_best`, the chunk's motion search results.
// dP: the chunk's parameters in device memory (what the kernels read; n_frames and the loop-filter levels are not used by them),
// followed with adaptive quantisation by the quantiser slots' copies.  The kernels get P's split masks and quantiser indices from the
// launch's first frame on.
// sym_order (key frames, frame0 = 0, with sym_count: 16 zeroed counters): every tile of the launch adds itself to its weight class's row
// of sym_order[AV1MI_TILE_CLASSES][count x tiles per frame] (tile_weight_rule.h), for av1mi_launch_entropy over the same frames; or null.
hipError_t av1mi_launch_recon_u16(const Av1miDevParams *P, const Av1miDevParams *dP, const void *src, void *rec, int16_t *levels, Av1miBlkInfo *blk,
                                  const void *fin, const unsigned long long *me_best, int frame0, int count, uint32_t *sym_count, uint32_t *sym_order, hipStream_t stream);
hipError_t av1mi_launch_recon_u8(const Av1miDevParams *P, const Av1miDevParams *dP, const void *src, void *rec, int16_t *levels, Av1miBlkInfo *blk,
                                 const void *fin, const unsigned long long *me_best, int frame0, int count, uint32_t *sym_count, uint32_t *sym_order, hipStream_t stream);
hipError_t av1mi_launch_recon64_u16(const Av1miDevParams *P, const Av1miDevParams *dP, const void *src, void *rec, int16_t *levels, Av1miBlkInfo *blk,
                                    const void *fin, const unsigned long long *me_best, int frame0, int count, uint32_t *sym_count, uint32_t *sym_order, hipStream_t stream);
hipError_t av1mi_launch_recon64_u8(const Av1miDevParams *P, const Av1miDevParams *dP, const void *src, void *rec, int16_t *levels, Av1miBlkInfo *blk,
                                   const void *fin, const unsigned long long *me_best, int frame0, int count, uint32_t *sym_count, uint32_t *sym_order, hipStream_t stream);
// both passes over the frames of `rec`, in place, with the levels of frame0's kind (av1mi_frame_lf_levels) or, with the level search
// on, each frame's own (P->lf_sel: av1mi_launch_deblock_search on the same stream before)
hipError_t av1mi_launch_deblock(const Av1miDevParams *P, void *rec, const Av1miBlkInfo *blk, int frame0, int count, hipStream_t stream);
// the level search on the frames of `rec` before deblocking (P->lf_err zeroed by the caller), then the decision: the frames' levels into
// P->lf_sel and into their headers
hipError_t av1mi_launch_deblock_search(const Av1miDevParams *P, const void *rec, const void *src, const Av1miBlkInfo *blk, uint8_t *hdr_blob,
                                       int frame0, int count, hipStream_t stream);
// the strength search (P->cdef_err zeroed by the caller), then the selection; one-frame launches (the P-frame chain) in 8-row strips, as CDEF
hipError_t av1mi_launch_cdef_search(const Av1miDevParams *P, const void *rec, const void *src, const Av1miBlkInfo *blk, uint8_t *hdr_blob,
                                    int frame0, int count, hipStream_t stream);
// `rec` filtered into `fin` (the caller's choice of output array).  src and sse, both or neither: the squared error of the output against
// the source is added to sse[frame][plane] - launches of several frames only (a one-frame launch sits on an inter chunk's serial chain:
// it runs in strips and cannot sum it)
hipError_t av1mi_launch_cdef(const Av1miDevParams *P, const void *rec, void *fin, const Av1miBlkInfo *blk, const void *src,
                             unsigned long long *sse, int frame0, int count, hipStream_t stream);
// choice and unit_sse: [frame][plane][unit] (av1mi_lr_frame_units per frame), unit_sse with 8 sums per unit - scratch of the two phases,
// cleared here for the launch's frames with `clear`, else by the caller (the frame loop of a P chunk clears the whole chunk's once
// instead of putting a fill between every frame's kernels on the chain)
// decide = 0: phase 0 alone - the fixed candidates' sums, for av1mi_launch_lr_fit on the same stream to decide with
hipError_t av1mi_launch_lr(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                           unsigned long long *unit_sse, int clear, int decide, int frame0, int count, hipStream_t stream);
// the self-guided fit (lr_fit_kernel.hip), after av1mi_launch_lr with decide = 0: sums, exact SSE, decision and filter, unit codes.
// fit: the chunk-wide buffers, cleared by the caller once per attempt at the chunk; choice gets 0 .. 22
hipError_t av1mi_launch_lr_fit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                               const unsigned long long *unit_sse, const Av1miLrFit *fit, int frame0, int count, hipStream_t stream);
// the Wiener fit (lr_wfit_kernel.hip), after the decision and application above (av1mi_launch_lr with decide = 1, or av1mi_launch_lr_fit):
// sums, solve and exact SSE, the override of units the fitted filter improves, and every Wiener unit's code.  sgr_fit: the self-guided
// fit's buffers when it ran (the winner's error is then its err[choice]), else null (unit_sse[choice]).  wfit: the chunk-wide buffers,
// cleared by the caller once per attempt at the chunk; choice gets 23 where the fitted filter won
hipError_t av1mi_launch_lr_wfit(const Av1miDevParams *P, const void *pre, const void *cdef, const void *src, void *out, uint8_t *choice,
                                const unsigned long long *unit_sse, const Av1miLrFit *sgr_fit, const Av1miLrWfit *wfit, int frame0, int count,
                                hipStream_t stream);
// tile_order: n_tiles entries of scratch.  mid: recorded on `stream` after symbolize, or null.  aux != null: the frame-edge tiles'
// symbolize variant runs there, beside the regular one, between `fork` and `join`.  cdf_init: Av1miCdfCompact::BLOB_WORDS entries, 16-byte
// aligned - the blob (Av1miCdfLayout) and behind it its compact image for P->max_bs_log2 (av1mi_cdf_compact_build)
// sym_count, sym_order: what av1mi_launch_recon filled for the same frames (frame0 = 0, key frames only, one-superblock tiles) - the
// regular symbolize variant takes its tiles from the heaviest class down; null: natural order.  Every other variant keeps natural order.
hipError_t av1mi_launch_entropy(const Av1miDevParams *P, const uint16_t *cdf_init, const int16_t *levels, const Av1miBlkInfo *blk,
                                uint32_t *streams, uint32_t *stream_len, uint32_t *tile_combos, uint8_t *slots, uint32_t *tile_bytes,
                                const uint8_t *lr_choice, uint32_t *tile_order, const uint32_t *sym_count, const uint32_t *sym_order,
                                int frame0, int count, hipStream_t stream, hipEvent_t mid, hipStream_t aux, hipEvent_t fork, hipEvent_t join);
}

// 64x64 leaf blocks run the kernels of recon64_kernel.hip (64-point transforms, larger LDS tiles)
inline hipError_t av1mi_launch_recon(const Av1miDevParams *P, const Av1miDevParams *dP, const void *src, void *rec, int16_t *levels, Av1miBlkInfo *blk,
                                     const void *fin, const unsigned long long *me_best, int frame0, int count, uint32_t *sym_count,
                                     uint32_t *sym_order, hipStream_t stream) {
  return (P->max_bs_log2 >= 6 ? (P->bit_depth == 8 ? av1mi_launch_recon64_u8 : av1mi_launch_recon64_u16)
                              : (P->bit_depth == 8 ? av1mi_launch_recon_u8 : av1mi_launch_recon_u16))(P, dP, src, rec, levels, blk, fin, me_best, frame0, count,
                                                                                                      sym_count, sym_order, stream);
}

#endif
