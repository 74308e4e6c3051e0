// av1mi_host.cpp - one chunk through the encoder, behind av1mi_encode_chunk of include/av1mi.h: prepare_chunk, the schedule of the
// chunk's kind, packing, download_chunk.  (The parameters and headers are av1mi_syntax.cpp's, the context and its workspace
// av1mi_ctx.cpp's.)
//
// Mirrors the reference's encode boundary: `run_av1an(&Av1anEncodeParams) -> Result<(), EncodeError>`
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139) becomes av1mi_encode_file(); the
// per-chunk work av1an farms out to SVT-AV1 workers (`--workers`, av1an.rs:100-101) becomes
// av1mi_encode_chunk() on one context (= one GPU + one HIP stream).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "av1mi_ctx.h"
#include "lr_fit_rule.h"
#include "wiener_fit_rule.h"
#include "deblock_pieces.h"
#include "part_inter_rule.h"
#include "tpl_rule.h"
#include "fg_rule.h"
#include "fg_synth_rule.h"

using namespace av1mi;

extern "C" {

// ---- one chunk: prepare_chunk, the schedule of its kind with entropy coding inside, packing, download_chunk
// Header blob, CDFs, parameters and clears, then the source frames - uploaded, and edge-extended where the coded size is not the
// signalled one - and their partition.  *d_src: the chunk's source frames on the device, at the coded size.
static int prepare_chunk(av1mi_ctx *c, const Resolved &r, const void *frames, uint32_t n_frames, int frames_on_device, const void **d_src) {
  Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s = c->stream;
  // header blob: sequence header OBU, then one fixed-size slot per frame with that frame's header (key and inter
  // frames have different lengths; frames of one kind differ only in grain_seed)
  size_t str_key = 0, str_inter = 0;   // CDEF strength search: where cdef_select_kernel writes each frame's set
  size_t lf_key = 0, lf_inter = 0;     // deblocking level search: where deblock_decide_kernel writes each frame's levels
  size_t fg_bit[2] = { 0, 0 };         // film-grain estimate: where fg_table_kernel writes each frame's table (key, inter)
  size_t ar_bit[2] = { 0, 0 };         // ... and fg_ar_solve_kernel the autoregressive coefficients
  size_t q_bit[2] = { 0, 0 };          // the frame term: where aq_map_kernel writes each frame's base_q_idx
  std::vector<uint8_t> seq = make_sequence_header(r), fh = make_frame_header(r, nullptr, 0, false, &str_key, &lf_key, &fg_bit[0], &ar_bit[0], &q_bit[0]),
                       fhi = make_frame_header(r, nullptr, 0, true, &str_inter, &lf_inter, &fg_bit[1], &ar_bit[1], &q_bit[1]);
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
  // deblocking level search (deblock_decide_kernel writes the levels), the film-grain estimate (fg_table_kernel writes the table) and
  // the frame term (aq_map_kernel writes the frames' base_q_idx).
  if (w.hdr_bytes != blob.size() || memcmp(w.h_hdr, blob.data(), blob.size())) {
    w.hdr_bytes = 0;
    memcpy(w.h_hdr, blob.data(), blob.size());
    HIPCHK(c, hipMemcpyAsync(w.d_hdr, w.h_hdr, blob.size(), hipMemcpyHostToDevice, s));
  }
  w.hdr_bytes = P.cdef_search || P.lf_search || r.fg_estimate || r.fq ? 0 : blob.size();
  // the default CDFs of the chunk's q context - or, with the frame term, of all four one after the other: a frame's tiles take the
  // blob of its own q_f (entropy_kernel.hip: frame_cdf) - once per context and leaf size
  const int cdf_key = r.fq ? AV1MI_CDF_ALL : r.qidx;
  if (w.cdf_qidx != cdf_key || w.cdf_bs_log2 != P.max_bs_log2) {
    w.cdf_qidx = -1;
    static const int context_qidx[4] = { 20, 60, 120, 255 };   // an index of each q context (av1mi_q_context)
    const int n_blobs = r.fq ? 4 : 1;
    for (int k = 0; k < n_blobs; k++) {
      // the blob, and behind it the regular symbolize variants' compact image of it for this leaf size (av1mi_dev.h: Av1miCdfCompact)
      std::vector<uint16_t> cdf = make_cdf_blob(r.fq ? context_qidx[k] : r.qidx);
      cdf.resize(Av1miCdfCompact::BLOB_WORDS, 0);
      av1mi_cdf_compact_build(cdf.data(), P.max_bs_log2, cdf.data() + Av1miCdfCompact::AT);
      memcpy(w.h_cdf + (size_t)k * Av1miCdfCompact::BLOB_WORDS, cdf.data(), cdf.size() * 2);
    }
    HIPCHK(c, hipMemcpyAsync(w.d_cdf, w.h_cdf, (size_t)n_blobs * Av1miCdfCompact::BLOB_WORDS * 2, hipMemcpyHostToDevice, s));
    w.cdf_qidx = cdf_key; w.cdf_bs_log2 = P.max_bs_log2;
  }
  {
    // The recon kernel reads its parameters from device memory: P, and with adaptive quantisation the quantiser slots' copies behind it
    const std::vector<Av1miDevParams> par = slot_params(P);
    const int n_par = (int)par.size();
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
  if (c->quality) HIPCHK(c, hipMemsetAsync(w.d_quality, 0, (size_t)n_frames * 3 * 2 * sizeof(unsigned long long), s));   // the quality pass adds
  if (displayed_on(c, r)) HIPCHK(c, hipMemsetAsync(w.d_disp_quality, 0, (size_t)n_frames * 3 * 2 * sizeof(unsigned long long), s));
  HIPCHK(c, hipEventRecord(c->ev[EV_START], s));
  // the caller's frames are used in place if they are on the device at the coded size; a padded chunk arrives in the stage, and so does
  // a chunk the film-grain denoiser will write d_src from - and, for the displayed picture's quality, one whose key frames the temporal
  // filter will rewrite in d_src: the pass compares against the frames as the caller gave them
  const bool staged = r.padded || r.fg_denoise || (displayed_on(c, r) && tf_runs(r, n_frames));
  if (!frames_on_device) HIPCHK(c, hipMemcpyAsync(staged ? w.d_stage : w.d_src, frames, caller_bytes(r, n_frames), hipMemcpyHostToDevice, s));
  const void *tight = frames_on_device ? frames : w.d_stage;   // (with `staged`) the frames as the caller gave them, on the device
  // not a multiple of 8: edge-extend every frame to the coded size (the signalled size stays exact)
  if (r.padded) HIPCHK(c, av1mi_launch_pad(tight, w.d_src, (int)r.p.width, (int)r.p.height, r.cw, r.ch, P.bit_depth, (int)n_frames, 0, s));
  *d_src = r.padded ? w.d_src : (staged ? tight : (frames_on_device ? frames : w.d_src));
  c->d_orig = frames_on_device || staged ? tight : w.d_src;   // (nothing writes the stage before the chunk's last kernels have read it)
  // the grain passes.  The film-grain estimate: the table from the frames as the caller gave them - before the denoiser and the temporal
  // filter - into every frame header, in front of every other kernel that patches a header (neighbouring fields can share a byte).  The
  // grain's autoregressive fit on the same frames: the coefficients, and the table scaled by the fit's gains over fg_table_kernel's values,
  // into every frame header.  The denoiser: the caller's frames filtered by the estimate's table into d_src at the coded size - out of place,
  // the edge extension in its store (a padded chunk's extension above served the estimate alone) - with the temporal term behind the search
  // of every frame in its neighbours, which reads the undenoised *d_src first.  Everything below reads the denoised chunk
  if (r.fg_estimate) {
    const Av1miFgBits bits = { (int)fg_bit[0], (int)fg_bit[1], (int)ar_bit[0], (int)ar_bit[1] };
    HIPCHK(c, launch_grain_passes(P, r, tight, *d_src, w.d_fg, w.d_fg_ar, w.d_src, w.d_hdr, bits, s, w.d_fgd_mv));
    if (r.fg_denoise) *d_src = w.d_src;
  }
  // the key frames' temporal filter: in place in the chunk's source - a chunk that is used in place is copied first, the caller's
  // memory is never written.  Everything below and after reads the filtered key frames.
  if (tf_runs(r, n_frames)) {
    if (*d_src != w.d_src) { HIPCHK(c, hipMemcpyAsync(w.d_src, *d_src, caller_bytes(r, n_frames), hipMemcpyDeviceToDevice, s)); *d_src = w.d_src; }
    HIPCHK(c, av1mi_launch_temporal_filter(&P, w.d_src, w.d_tf_mv, r.tf_frames, r.tf_strength, s));
  }
  // content-driven partition: the split masks of every superblock of the chunk, from the source, before anything walks blocks (the second
  // stream's motion search waits for EV_SRC_READY as well)
  if (P.part_map) HIPCHK(c, av1mi_launch_partition(&P, *d_src, w.d_part, s));
  // adaptive quantisation: every superblock's quantiser index, likewise from the source and on the device - the walks and symbolize read the map
  // ... with a temporal strength behind the chunk's temporal-dependency analysis (it sees the filtered key frames): beta of every
  // superblock and the chunk's sum of it, the flow cleared once per attempt at the chunk
  // ... and with a frame strength behind the frames' sums of the same analysis (which it runs whatever the temporal strength): every
  // frame's base_q_idx, into the map, into P.frame_q and into the frame's header - all on the device, no host round trip in front of
  // "source ready"
  const unsigned long long *beta_sum = nullptr;
  Av1miFqMap fq = {};
  if (r.tpl || r.fq) {
    const size_t n_flow = av1mi_tpl_flow_entries(r.cw, r.ch, (int)n_frames);
    HIPCHK(c, hipMemsetAsync(w.d_tpl_flow, 0, n_flow * sizeof(unsigned long long), s));
    HIPCHK(c, av1mi_launch_tpl(&P, *d_src, w.d_tpl_intra, w.d_tpl_inter, w.d_tpl_key, w.d_tpl_flow, w.d_tpl_beta, s));
    beta_sum = w.d_tpl_flow + n_flow - 1;
  }
  if (r.fq) {
    fq.strength = r.fq; fq.q_bit[0] = (int)q_bit[0]; fq.q_bit[1] = (int)q_bit[1];
    fq.fq = av1mi_fq_split(w.d_fq, n_frames); fq.hdr_blob = w.d_hdr;
    HIPCHK(c, av1mi_launch_tpl_frames(&P, w.d_tpl_intra, w.d_tpl_flow, w.d_tpl_beta, fq.fq, s));
  }
  if (P.aq_map) HIPCHK(c, av1mi_launch_aq(&P, *d_src, w.d_aq_act, w.d_aq_map, r.aq, w.d_tpl_beta, r.tpl ? beta_sum : nullptr, r.tpl, &fq, s));
  HIPCHK(c, hipEventRecord(c->ev[EV_SRC_READY], s));
  return AV1MI_OK;
}

// Whether symbolize takes this chunk's tiles heavy first: all-key-frame chunks with one-superblock tiles, adaptive CDFs and
// leaves up to 32x32, unless AV1MI_SYM_ORDER = 0.  The reconstruction launch then fills the table and symbolize reads it; run_chunk
// remembers its tiles for av1mi_sym_order_result.  (64x64 leaves: measured, the reconstruction wave's wait for its place in the table - it
// has just stored a whole superblock - costs that launch 0.034 ms, more than symbolize gains: DESIGN 5h.)
static bool sym_order_on(const av1mi_ctx *c) { return c->sym_order && c->P.tile_sb == 1 && !c->P.disable_cdf_update && c->P.max_bs_log2 <= 5; }

// The entropy coder's parameters: the chunk's - without the map where the stream carries no deltas: with the frame term alone the map
// holds the frames' q_f for the reconstruction's slots, delta_q_present is 0 and symbolize codes none.
static Av1miDevParams entropy_params(const av1mi_ctx *c) {
  Av1miDevParams E = c->P;
  if (!dq_on(c->ws.res)) E.aq_map = nullptr;
  return E;
}

// Entropy coding of frames [from, n_frames) on the main stream (the frame-edge tiles' symbolize variant on the fourth), then the join
// with the groups of frames before `from` coded on the third (schedule_inter): packing needs the tile sizes and bytes of every frame.
// by_weight: symbolize takes the tiles in the order the chunk's reconstruction launch left (sym_order_on).
static int entropy_code(av1mi_ctx *c, uint32_t from, uint32_t n_frames, bool by_weight = false) {
  Workspace &w = c->ws; hipStream_t s = c->stream;
  const Av1miDevParams E = entropy_params(c);
  HIPCHK(c, hipEventRecord(c->ev[EV_RECON_DONE], s));
  HIPCHK(c, av1mi_launch_entropy(&E, w.d_cdf, w.d_levels, w.d_blk, w.d_streams, w.d_sym, w.d_combos, w.d_slots, w.d_tile_bytes, w.d_lrc,
                                 w.d_tile_off /* scratch until the packing kernels fill it */, by_weight ? w.d_sym_count : nullptr,
                                 by_weight ? w.d_sym_order : nullptr, (int)from, (int)(n_frames - from),
                                 s, c->ev[EV_SYM_DONE], c->stream4, c->ev[EV_EDGE_FORK], c->ev[EV_EDGE_JOIN]));
  if (from) HIPCHK(c, hipStreamWaitEvent(s, c->ev[EV_GROUPS_JOINED], 0));
  HIPCHK(c, hipEventRecord(c->ev[EV_ENTROPY_DONE], s));
  return AV1MI_OK;
}

// The chunk's planes as the quality pass sees them: stored at the coded size, compared over the signalled one
static Av1miQualityGeom quality_geom(const Av1miDevParams &P) { return av1mi_quality_geom(P.true_w, P.true_h, P.width, P.height, P.bit_depth); }

// With the context's quality switch on: the final frames against the coded source, one launch over the chunk on the second stream behind
// the squared error's (off: nothing)
static int quality_beside_sse(av1mi_ctx *c, const void *src) {
  if (!c->quality) return AV1MI_OK;
  const Av1miQualityGeom G = quality_geom(c->P);
  HIPCHK(c, av1mi_launch_quality(&G, src, c->ws.d_fin, c->P.n_frames, c->ws.d_quality, nullptr, c->stream2));
  return AV1MI_OK;
}

// With the displayed-quality switch on and film grain in the headers: what a decoder shows - the final frames with the grain of the
// headers' parameters and seeds, which fgs_params_kernel reads where the estimate and the fit left them - into d_disp in the caller's
// layout, then the quality pass of that against the frames as the caller gave them; on the second stream behind the squared error's
static int displayed_beside_sse(av1mi_ctx *c) {
  const Resolved &r = c->ws.res;
  if (!displayed_on(c, r)) return AV1MI_OK;
  const Av1miDevParams &P = c->P; Workspace &w = c->ws; hipStream_t s2 = c->stream2;
  const Av1miFgsBlock B = av1mi_fgs_split(w.d_fgs, (size_t)P.n_frames);
  const uint8_t *table = !r.fg_estimate ? nullptr : (r.fg_ar_lag ? av1mi_fgar_split(w.d_fg_ar).table : av1mi_fg_split(w.d_fg).table);
  const Av1miQualityGeom coded = quality_geom(P), tight = av1mi_quality_geom(P.true_w, P.true_h, P.true_w, P.true_h, P.bit_depth);
  HIPCHK(c, av1mi_launch_fg_synth_params((int)r.p.film_grain, r.fg_estimate, r.fg_ar_lag, table, r.fg_ar_lag ? av1mi_fgar_split(w.d_fg_ar).coeffs : nullptr, B, s2));
  HIPCHK(c, av1mi_launch_fg_synth_templates(P.bit_depth, P.true_w, P.true_h, P.n_frames, nullptr, r.p.first_frame, B, s2));
  HIPCHK(c, av1mi_launch_fg_synth_apply(&coded, &tight, w.d_fin, w.d_disp, P.n_frames, B, s2));
  HIPCHK(c, av1mi_launch_quality(&tight, c->d_orig, w.d_disp, P.n_frames, w.d_disp_quality, nullptr, s2));
  return AV1MI_OK;
}

// The second stream beside the range coder, once symbolize is done: the squared error of the final frames
static int sse_beside_range_coder(av1mi_ctx *c, const void *src) {
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev[EV_SYM_DONE], 0));
  HIPCHK(c, hipEventRecord(c->ev[EV_CDEF_START], c->stream2));
  HIPCHK(c, av1mi_launch_sse(&c->P, src, c->ws.d_fin, c->ws.d_sse, c->stream2));
  if (const int rc = quality_beside_sse(c, src)) return rc;
  if (const int rc = displayed_beside_sse(c)) return rc;
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
  const bool by_weight = sym_order_on(c);
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
  if (const int rc = quality_beside_sse(c, src)) return rc;
  if (const int rc = displayed_beside_sse(c)) return rc;
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
  const bool by_weight = sym_order_on(c);
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
      const Av1miDevParams E = entropy_params(c);
      HIPCHK(c, av1mi_launch_entropy(&E, w.d_cdf, w.d_levels, w.d_blk, w.d_streams, w.d_sym, w.d_combos, w.d_slots, w.d_tile_bytes, w.d_lrc,
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
  if (e1 == hipSuccess && c->quality) e1 = hipMemcpyAsync(w.h_quality, w.d_quality, (size_t)n_frames * 3 * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && displayed_on(c, r)) e1 = hipMemcpyAsync(w.h_disp_quality, w.d_disp_quality, (size_t)n_frames * 3 * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  // the level search's tables and levels (record_last_chunk keeps them): one more small copy before the wait below.  The levels sit behind the
  // whole workspace's tables, not behind this chunk's: two copies when the chunk is shorter
  const size_t lf_err_bytes = (size_t)n_frames * 3 * AV1MI_LF_CANDS * sizeof(unsigned long long);
  if (e1 == hipSuccess && P.lf_search) e1 = hipMemcpyAsync(w.h_lf, w.d_lf_err, lf_err_bytes, hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && P.lf_search) e1 = hipMemcpyAsync(w.h_lf + lf_err_bytes, w.d_lf_sel, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s);
  // the film-grain estimate's table and counts, likewise
  if (e1 == hipSuccess && r.fg_estimate) e1 = hipMemcpyAsync(w.h_fg, w.d_fg, av1mi_fg_result_bytes(), hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && r.fg_ar_lag) e1 = hipMemcpyAsync(w.h_fg_ar, w.d_fg_ar, av1mi_fgar_result_bytes(), hipMemcpyDeviceToHost, s);
  // the frame term's block, likewise
  if (e1 == hipSuccess && r.fq) e1 = hipMemcpyAsync(w.h_fq, w.d_fq, av1mi_fq_bytes(n_frames), hipMemcpyDeviceToHost, s);
  // the self-guided fit's errors and records, likewise
  const size_t fit_n = (size_t)n_frames * 3 * av1mi_lr_unit_rows(P) * av1mi_lr_unit_cols(P);
  if (e1 == hipSuccess && P.lr_fit_code) e1 = hipMemcpyAsync(w.h_fit, w.d_fit, av1mi_lr_fit_result_bytes(fit_n), hipMemcpyDeviceToHost, s);
  if (e1 == hipSuccess && P.lr_wfit_code) e1 = hipMemcpyAsync(w.h_wfit, w.d_wfit, av1mi_lr_wfit_result_bytes(fit_n), hipMemcpyDeviceToHost, s);
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

// What the context reports of the chunk it has just encoded (av1mi_ctx.cpp's *_result, *_units and *_tiles entry points): the small
// results download_chunk brought to the host, and what tells where the larger ones still stand on the device.
static LastChunk record_last_chunk(const av1mi_ctx *c, const Resolved &r, uint32_t n_frames, bool inter) {
  const Av1miDevParams &P = c->P; const Workspace &w = c->ws;
  LastChunk L;
  L.n_frames = n_frames;
  L.lf_levels.resize((size_t)n_frames * 4);
  L.lf_errs.assign((size_t)n_frames * 3 * AV1MI_LF_CANDS, 0);
  if (P.lf_search) {   // (the levels sit behind this chunk's tables in h_lf)
    const size_t lf_err_bytes = (size_t)n_frames * 3 * AV1MI_LF_CANDS * sizeof(unsigned long long);
    memcpy(L.lf_errs.data(), w.h_lf, lf_err_bytes);
    memcpy(L.lf_levels.data(), w.h_lf + lf_err_bytes, (size_t)n_frames * 4);
  } else {
    for (uint32_t f = 0; f < n_frames; f++) for (int i = 0; i < 4; i++) L.lf_levels[(size_t)f * 4 + i] = (uint8_t)av1mi_frame_lf_levels(P, (int)f)[i];
  }
  L.fit_plane_units = (uint32_t)(av1mi_lr_unit_rows(P) * av1mi_lr_unit_cols(P));
  L.fit_units = (size_t)n_frames * 3 * L.fit_plane_units;
  L.fit_on = P.lr_fit_code != nullptr;   // (the values stay in h_fit until the context's next chunk)
  L.wfit_on = P.lr_wfit_code != nullptr;
  if (!inter && sym_order_on(c)) L.sym_tiles = n_frames * (uint32_t)(P.tile_rows * P.tile_cols);   // (the all-key schedules' table)
  if (r.fg_estimate) memcpy(L.fg_table, av1mi_fg_split(w.h_fg).table, sizeof(L.fg_table));   // (the fetched heads of the two blocks)
  if (r.fg_ar_lag) {   // the headers carry the scaled table
    const Av1miFgArBlock H = av1mi_fgar_split(w.h_fg_ar);
    memcpy(L.fg_table, H.table, sizeof(L.fg_table));
    memcpy(L.fg_ar_coeffs, H.coeffs, sizeof(L.fg_ar_coeffs));
    memcpy(L.fg_sigma_table, H.sigma, sizeof(L.fg_sigma_table));
    memcpy(L.fg_ar_gain, H.gain, sizeof(L.fg_ar_gain));
  }
  L.frame_q.assign(n_frames, (uint8_t)r.qidx);
  L.frame_beta.assign(n_frames, 0);
  if (r.fq) {
    const Av1miFqBlock H = av1mi_fq_split(w.h_fq, n_frames);
    memcpy(L.frame_q.data(), H.frame_q, n_frames);
    memcpy(L.frame_beta.data(), H.beta, (size_t)n_frames * sizeof(uint16_t));
  }
  L.quality.assign((size_t)n_frames * 3, av1mi_plane_quality{});
  if (c->quality) {
    const Av1miQualityGeom G = quality_geom(P);
    for (size_t i = 0; i < L.quality.size(); i++) L.quality[i] = plane_quality(w.h_quality + i * 2, G, (int)(i % 3));
  }
  L.displayed.assign((size_t)n_frames * 3, av1mi_plane_quality{});
  if (displayed_on(c, r)) {
    const Av1miQualityGeom G = av1mi_quality_geom(P.true_w, P.true_h, P.true_w, P.true_h, P.bit_depth);
    for (size_t i = 0; i < L.displayed.size(); i++) L.displayed[i] = plane_quality(w.h_disp_quality + i * 2, G, (int)(i % 3));
  }
  L.film_grain = r.p.film_grain; L.fg_estimate = r.fg_estimate != 0; L.fg_ar_lag = r.fg_ar_lag;
  if (P.part_map) { L.pi_keys = c->part_inter; L.pi_frames = n_frames; L.pi_units = (uint32_t)(P.b8_rows * P.b8_cols); L.pi_sbs = (uint32_t)(P.sb_rows * P.sb_cols); }
  return L;
}

static int run_chunk(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                     av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report) {
  out->data = nullptr; out->size = 0;
  c->last = LastChunk();
  Resolved r;
  int rc = resolve(params, &r);
  if (rc) { set_err(c, "invalid parameters"); return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_workspace(c, r, n_frames);
  if (rc) return rc;
  Workspace &w = c->ws;
  c->P = dev_params(r, n_frames, c->cap_scale);
  bind_workspace(c->P, r, w);
  c->part_inter = r.p.partition_search == 2 && c->P.keyint > 1 && n_frames > 1;   // (the chunk goes through schedule_inter)
  const void *d_src = nullptr;
  rc = prepare_chunk(c, r, frames, n_frames, frames_on_device, &d_src);
  if (rc) return rc;
  const Av1miDevParams &P = c->P;
  const bool inter = P.keyint > 1 && n_frames > 1;
  if (inter) rc = schedule_inter(c, d_src, n_frames);
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
  if (rc == AV1MI_OK) c->last = record_last_chunk(c, r, n_frames, inter);
  return rc;
}

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

int av1mi_encode_chunk(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                       av1mi_buf *out, uint32_t *frame_sizes, void *recon, av1mi_report *report) {
  if (!c || !frames || !out || n_frames == 0) return AV1MI_E_INVALID_ARG;
  for (;;) {
    const int rc = encode_chunk_once(c, params, frames, n_frames, frames_on_device, out, frame_sizes, recon, report);
    if (rc != AV1MI_E_OVERFLOW || c->cap_scale >= 64) return rc;
    c->cap_scale *= 2;  // stays raised for the following chunks of this context (same content)
  }
}

}  // extern "C"
