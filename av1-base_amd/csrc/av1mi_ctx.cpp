// av1mi_ctx.cpp - the context of libav1mi's C ABI (include/av1mi.h) and what it owns: workspace, stream pool, page-locked block
// pool, the stand-alone passes on buffers of their own, and what the context reports of its last chunk.  No CPU encode path exists
// here: without a HIP device every entry point fails with AV1MI_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "av1mi_ctx.h"
#include "lr_fit_rule.h"
#include "lr_rate_rule.h"
#include "wiener_fit_rule.h"
#include "deblock_pieces.h"
#include "aq_rule.h"
#include "tpl_rule.h"
#include "fg_rule.h"
#include "fg_ar_rule.h"
#include "fg_denoise_rule.h"
#include "fg_synth_rule.h"
#include "part_inter_rule.h"

namespace av1mi {

void set_err(av1mi_ctx *c, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
}

void free_workspace(av1mi_ctx *c) {
  for (auto &b : c->ws.owned) (void)(b.second ? hipHostFree(b.first) : hipFree(b.first));
  c->ws = Workspace();
}

// a buffer that grows on need: (re)allocated when a chunk needs more than it holds; `bytes` is 0 while it holds nothing usable
template <class T>
static hipError_t ws_grow(Workspace &w, T *&p, size_t &bytes, size_t need) {
  if (bytes >= need) return hipSuccess;
  bytes = 0;
  const hipError_t e = ws_alloc(w, p, need);
  if (e == hipSuccess) bytes = need;
  return e;
}

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
    // the small blocks that have a page-locked mirror on the host: header blob, default CDFs with their compact image, parameters,
    // chunk record with frame_off[nf + 1], squared errors
    // (CDFs and parameters at what the frame term needs - four q contexts, 28 quantiser slots: 50 KB; a chunk uploads what it uses)
    const size_t hdr_bytes = 256 + nf * 512, cdf_bytes = 4 * Av1miCdfCompact::BLOB_WORDS * sizeof(uint16_t), par_bytes = AV1MI_FQ_SLOTS * sizeof(Av1miDevParams),
                 rec_bytes = sizeof(Av1miChunkRecord) + (nf + 1) * 8, sse_bytes = nf * 3 * 8;
    for (void **b : { &w.d_src, &w.d_rec, &w.d_fin }) HIPCHK(c, ws_alloc(w, *b, nf * frame_bytes));
    HIPCHK(c, ws_alloc(w, w.d_levels, nf * nsb * AV1MI_SB_LEVELS * sizeof(int16_t)));
    HIPCHK(c, ws_alloc(w, w.d_blk, nf * nb8 * sizeof(Av1miBlkInfo)));
    // on the context's own stream: hipMemset would run on the null stream, which a non-blocking stream does not wait
    // for - the fill could land after the first reconstruction kernel had written its block info
    HIPCHK(c, hipMemsetAsync(w.d_blk, 0, nf * nb8 * sizeof(Av1miBlkInfo), c->stream));
    HIPCHK(c, ws_alloc(w, w.d_slots, nf * ntile * slot * 2));  // 16-bit pre-carry entries, one per output byte
    w.out_cap = nf * (ntile * (slot + 4) + 256);
    HIPCHK(c, ws_alloc(w, w.d_out, w.out_cap));
    HIPCHK(c, ws_alloc(w, w.d_hdr, hdr_bytes));
    HIPCHK(c, ws_alloc(w, w.d_cdf, cdf_bytes));
    HIPCHK(c, ws_alloc(w, w.d_params, par_bytes));
    for (uint32_t **b : { &w.d_tile_bytes, &w.d_tile_off, &w.d_sym, &w.d_combos }) HIPCHK(c, ws_alloc(w, *b, nf * nsb * 4));
    HIPCHK(c, ws_alloc(w, w.d_streams, nf * ntile * (size_t)tile_stream_cap(r, c->cap_scale) * 4));
    for (uint32_t **b : { &w.d_frame_size, &w.d_payload }) HIPCHK(c, ws_alloc(w, *b, nf * 4));
    HIPCHK(c, ws_alloc(w, w.d_record, rec_bytes));
    HIPCHK(c, ws_alloc(w, w.d_sym_count, AV1MI_TILE_CLASSES * 4 + sse_bytes));
    w.d_sse = reinterpret_cast<unsigned long long *>(w.d_sym_count + AV1MI_TILE_CLASSES);
    HIPCHK(c, ws_alloc(w, w.d_sym_order, (size_t)AV1MI_TILE_CLASSES * nf * ntile * 4));
    {  // the five small host mirrors share one page-locked block: an allocation of page-locked memory costs far more than they hold
      auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
      const size_t b_hdr = up(hdr_bytes), b_cdf = up(cdf_bytes), b_par = up(par_bytes), b_rec = up(rec_bytes), b_sse = up(sse_bytes);
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
  const size_t unit_cap = 3 * nf * nsb + 64;   // restoration units the choices, sums and fits have room for: three planes of 64x64 units
  // the caller's frames in front of a pass that writes d_src from them: the edge extension, and the film-grain denoiser at any size
  // ... and with the displayed picture's quality a chunk whose key frames the temporal filter rewrites in d_src
  if ((r.padded || r.fg_denoise || (displayed_on(c, r) && r.tf_frames)) && !w.d_stage) HIPCHK(c, ws_alloc(w, w.d_stage, caller_bytes(r, nf)));
  if (p.partition_search && !w.d_part) HIPCHK(c, ws_alloc(w, w.d_part, nf * nsb * sizeof(uint32_t)));
  if (p.me_presearch && !w.d_quarter) {
    HIPCHK(c, ws_alloc(w, w.d_quarter, nf * (size_t)(r.cw / 4) * (r.ch / 4) * sizeof(uint16_t)));
    HIPCHK(c, ws_alloc(w, w.d_centre, nf * nsb * sizeof(uint32_t)));
  }
  if (p.subpel && !w.d_me_sub) HIPCHK(c, ws_alloc(w, w.d_me_sub, nf * nb8 * 8));  // output of the sub-sample refinement
  if (p.block_log2 >= 6 && p.keyint > 1) {   // candidate table of the 64x64 leaves' motion search
    const size_t nc = 2 * (size_t)(p.me_range ? p.me_range : 8) + 1, need = nf * nsb * nc * nc * sizeof(uint32_t);
    HIPCHK(c, ws_grow(w, w.d_me64, w.me64_bytes, need));
  }
  if (p.partition_search == 2 && p.keyint > 1) {   // node tables of the inter frames' partition decision, on first use
    const size_t need = nf * av1mi_pi_frame_nodes(r.ch / 8, r.cw / 8) * sizeof(uint32_t);
    HIPCHK(c, ws_grow(w, w.d_nodes, w.nodes_bytes, need));
  }
  // the keys of the film-grain denoiser's temporal term, on first use (and when a chunk has more frames than any before)
  if (r.fg_denoise_span) HIPCHK(c, ws_grow(w, w.d_fgd_mv, w.fgd_mv_bytes, fgd_mv_entries(r, n_frames) * sizeof(uint32_t)));
  // the temporal filter's keys, on first use (and when a chunk has more key frames or followers than any before)
  if (r.tf_frames) HIPCHK(c, ws_grow(w, w.d_tf_mv, w.tf_mv_bytes, tf_mv_entries(r, n_frames) * sizeof(uint32_t)));
  if (qmap_on(r) && !w.d_aq_map) {
    HIPCHK(c, ws_alloc(w, w.d_aq_act, nf * nsb * sizeof(uint16_t)));
    HIPCHK(c, ws_alloc(w, w.d_aq_map, nf * nsb));
  }
  if (r.fq && (!w.d_fq || !w.h_fq)) {
    HIPCHK(c, ws_alloc(w, w.d_fq, av1mi_fq_bytes(nf)));
    HIPCHK(c, ws_alloc(w, w.h_fq, av1mi_fq_bytes(nf), true));
  }
  if ((r.tpl || r.fq) && !w.d_tpl_beta) {   // (beta last: every one of the five stands once it does)
    const size_t nb = (size_t)av1mi_tpl_blocks(r.cw) * av1mi_tpl_blocks(r.ch);
    for (uint32_t **b : { &w.d_tpl_intra, &w.d_tpl_inter, &w.d_tpl_key }) HIPCHK(c, ws_alloc(w, *b, nf * nb * sizeof(uint32_t)));
    HIPCHK(c, ws_alloc(w, w.d_tpl_flow, av1mi_tpl_flow_entries(r.cw, r.ch, (int)nf) * sizeof(unsigned long long)));
    HIPCHK(c, ws_alloc(w, w.d_tpl_beta, nf * nsb * sizeof(uint16_t)));
  }
  if (r.fg_estimate && (!w.d_fg || !w.h_fg)) {
    HIPCHK(c, ws_alloc(w, w.d_fg, av1mi_fg_bytes(fg_records(r, nf))));
    HIPCHK(c, ws_alloc(w, w.h_fg, av1mi_fg_result_bytes(), true));
  }
  if (r.fg_ar_lag && (!w.d_fg_ar || !w.h_fg_ar)) {
    HIPCHK(c, ws_alloc(w, w.d_fg_ar, av1mi_fgar_bytes()));
    HIPCHK(c, ws_alloc(w, w.h_fg_ar, av1mi_fgar_result_bytes(), true));
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
  if (c->quality && (!w.d_quality || !w.h_quality)) {
    HIPCHK(c, ws_alloc(w, w.d_quality, nf * 3 * 2 * sizeof(unsigned long long)));
    HIPCHK(c, ws_alloc(w, w.h_quality, nf * 3 * 2 * sizeof(unsigned long long), true));
  }
  if (displayed_on(c, r) && (!w.d_fgs || !w.d_disp || !w.d_disp_quality || !w.h_disp_quality)) {
    HIPCHK(c, ws_alloc(w, w.d_fgs, av1mi_fgs_bytes(nf, (size_t)av1mi_fgs_stripes((int)p.height) * av1mi_fgs_blocks((int)p.width))));
    HIPCHK(c, ws_alloc(w, w.d_disp, caller_bytes(r, nf)));
    HIPCHK(c, ws_alloc(w, w.d_disp_quality, nf * 3 * 2 * sizeof(unsigned long long)));
    HIPCHK(c, ws_alloc(w, w.h_disp_quality, nf * 3 * 2 * sizeof(unsigned long long), true));
  }
  if (p.enable_lr && !w.d_cd) {   // unit choices and sums for three planes (enable_lr 3 / 4) of 64x64 units, whichever value and unit size
                                  // this chunk has: the buffers stay with the geometry while enable_lr changes
    HIPCHK(c, ws_alloc(w, w.d_cd, nf * frame_bytes));
    HIPCHK(c, ws_alloc(w, w.d_lrc, unit_cap));
    HIPCHK(c, ws_alloc(w, w.d_lrsse, unit_cap * 8 * sizeof(unsigned long long)));
  }
  if (r.lr_fit_mask && (!w.d_fit || !w.h_fit)) {   // for three planes, like the unit sums: the buffers stay while enable_lr changes
    HIPCHK(c, ws_alloc(w, w.d_fit, av1mi_lr_fit_bytes(unit_cap)));
    HIPCHK(c, ws_alloc(w, w.h_fit, av1mi_lr_fit_result_bytes(unit_cap), true));
  }
  if (r.lr_fit_mask) w.fit = av1mi_lr_fit_split(w.d_fit, fit_chunk_units(r, n_frames), r.lr_fit_mask);   // this chunk's units, from the head of the block
  w.fit.mask = r.lr_fit_mask;
  if (r.lr_wfit && (!w.d_wfit || !w.h_wfit)) {
    HIPCHK(c, ws_alloc(w, w.d_wfit, av1mi_lr_wfit_bytes(unit_cap)));
    HIPCHK(c, ws_alloc(w, w.h_wfit, av1mi_lr_wfit_result_bytes(unit_cap), true));
  }
  if (r.lr_wfit) w.wfit = av1mi_lr_wfit_split(w.d_wfit, fit_chunk_units(r, n_frames));
  w.res = r;
  if (p.enable_qm && r.qm_level < 15) {
    // one slice of steps, or with adaptive quantisation one per quantiser slot (make_qm_table)
    if (!w.d_qm) HIPCHK(c, ws_alloc(w, w.d_qm, AV1MI_FQ_SLOTS * 2 * AV1MI_QM_PLANE * sizeof(Av1miQmEntry)));
    const int slices = quant_slots(r);
    const int key = (slices << 24) | (r.qm_level << 16) | (r.qidx << 4) | (int)p.bit_depth;
    if (w.qm_key != key) {
      w.h_qm = make_qm_table(r);
      HIPCHK(c, hipMemcpyAsync(w.d_qm, w.h_qm.data(), w.h_qm.size() * sizeof(Av1miQmEntry), hipMemcpyHostToDevice, c->stream));
      w.qm_key = key;
    }
  }
  return AV1MI_OK;
}

// The workspace's buffers bound into a chunk's parameters (dev_params leaves every pointer null): each where the chunk's kernels
// use it - the kernels take a null pointer for "off".
void bind_workspace(Av1miDevParams &P, const Resolved &r, const Workspace &w) {
  const av1mi_params &p = r.p;
  if (p.enable_qm && r.qm_level < 15) P.qm_tab = w.d_qm;
  if (p.partition_search) P.part_map = w.d_part;
  if (qmap_on(r)) P.aq_map = w.d_aq_map;
  if (r.fq) P.frame_q = av1mi_fq_split(w.d_fq, (size_t)P.n_frames).frame_q;
  if (p.cdef_search) { P.cdef_err = w.d_cdef_err; P.cdef_idx = w.d_cdef_idx; P.cdef_sel = w.d_cdef_sel; }
  if (p.deblock == 2) { P.lf_err = w.d_lf_err; P.lf_sel = w.d_lf_sel; }
  if (r.lr_fit_mask) P.lr_fit_code = w.fit.code;
  if (r.lr_wfit) P.lr_wfit_code = w.wfit.code;
  P.chunk_record = w.d_record; P.tile_symbols = w.d_sym;
}

hipError_t launch_grain_passes(const Av1miDevParams &P, const Resolved &r, const void *tight, const void *coded, uint8_t *d_fg, uint8_t *d_fg_ar, void *out,
                               uint8_t *hdr_blob, Av1miFgBits bits, hipStream_t s, uint32_t *d_mv, bool have_mv, bool estimate) {
  const Av1miFgBlock fg = av1mi_fg_split(d_fg);
  const int N = (int)r.p.film_grain;
  hipError_t e = hipSuccess;
  if (r.fg_estimate && coded && estimate) e = av1mi_launch_film_grain(&P, coded, fg, av1mi_fg_ceiling(N, 0), av1mi_fg_ceiling(N, 1), hdr_blob, bits, s);
  // (the table in d_fg stays as the estimate left it: the headers carry the fit's scaled one, the denoiser filters by the grain's whole sigma)
  if (e == hipSuccess && r.fg_ar_lag && coded && estimate && d_fg_ar) e = av1mi_launch_fg_ar(&P, coded, fg, r.fg_ar_lag, av1mi_fgar_split(d_fg_ar), hdr_blob, bits, s);
  const int span = r.fg_denoise ? r.fg_denoise_span : 0;
  if (e == hipSuccess && span && d_mv && !have_mv && coded) e = av1mi_launch_fg_denoise_search(&P, coded, d_mv, span, s);
  if (e == hipSuccess && r.fg_denoise && out) e = av1mi_launch_fg_denoise(&P, tight, out, fg.table, d_mv, span, s);
  return e;
}

}  // namespace av1mi

using namespace av1mi;

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
void av1mi::release_streams() {
  std::vector<std::pair<int, StreamSet>> all;
  { std::lock_guard<std::mutex> lk(g_stream_mu); all.swap(g_stream_pool); }
  for (auto &e : all) {
    (void)hipSetDevice(e.first);
    for (auto st : e.second.s) if (st) (void)hipStreamDestroy(st);
  }
}

// A context that goes back to av1mi_encode_file's cache forgets the capacity multiplier its last job's content raised (it would
// otherwise size - or, at the limit, refuse - an unrelated job's workspace by it); the next chunk reallocates at scale 1.
// ... and the quality switches a job set on it.
void av1mi::recycle_ctx(av1mi_ctx *c) { if (c) { c->cap_scale = 1; c->quality = false; c->displayed = false; } }

av1mi_plane_quality av1mi::plane_quality(const unsigned long long *q, const Av1miQualityGeom &G, int plane) {
  return { q[0], (int64_t)q[1], av1mi_quality_windows(G, plane), 0 };
}

extern "C" {

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
// count seen (expect_blocks) - freeing a block is hipHostFree, which synchronises the whole device
std::atomic<size_t> g_pin_free_max_blocks{16};
}  // namespace
}  // extern "C"

void *av1mi::pin_acquire(size_t bytes) {
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

void av1mi::expect_blocks(unsigned n) {
  size_t cur = g_pin_free_max_blocks.load();
  while (n > cur && n <= 256 && !g_pin_free_max_blocks.compare_exchange_weak(cur, n)) { }
}

void av1mi::release_buffers() {
  std::vector<std::pair<void *, size_t>> all;
  { std::lock_guard<std::mutex> lk(g_pin_mu); all.swap(g_pin_free); }
  for (auto &b : all) (void)hipHostFree(b.first);
}

extern "C" {

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

}  // extern "C"

namespace {

// A stand-alone pass's temporary device buffers and its first HIP error, after which every later step of the pass is skipped.
// Leaving the pass - by finish() or by any return before it - drains the stream first, also after a failure (nothing may still read
// or write the buffers), and then frees them.
struct PassBuffers {
  hipStream_t stream;
  hipError_t e = hipSuccess;
  std::vector<void *> owned;
  bool left = false;
  explicit PassBuffers(hipStream_t s) : stream(s) {}
  PassBuffers(const PassBuffers &) = delete;
  ~PassBuffers() { (void)leave(); }
  bool ok() const { return e == hipSuccess; }
  template <class T>
  bool alloc(T *&p, size_t bytes) {
    void *v = nullptr;
    if (ok() && (e = hipMalloc(&v, bytes)) == hipSuccess) owned.push_back(v);
    p = (T *)v;
    return ok();
  }
  hipError_t leave() {
    if (left) return hipSuccess;
    left = true;
    const hipError_t drained = hipStreamSynchronize(stream);
    for (void *b : owned) (void)hipFree(b);
    return drained;
  }
  // the end of the pass: what it returns, with the first error's text behind the pass's name in the context's message
  int finish(av1mi_ctx *c, const char *pass) {
    const hipError_t drained = leave();
    if (ok()) e = drained;
    if (ok()) return AV1MI_OK;
    set_err(c, "%s pass failed: %s", pass, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP;
  }
};

// What the stand-alone passes on frames at the coded size open with, after the null checks of their own arguments: the parameters
// resolved; then open() - the mode the pass needs (mode_on, of `r`, with what to say when it is off), the 16-byte alignment of the device
// pointers the caller gave (all of them or'ed, 0 for none), the context's device, and the kernels' parameters of the n frames as one
// chunk.  Until open() has succeeded the pass owns nothing and leaving it drains nothing.
struct Pass : PassBuffers {
  Resolved r = {};
  Av1miDevParams P;
  int rc;
  Pass(av1mi_ctx *c, const av1mi_params *params) : PassBuffers(c->stream), rc(resolve(params, &r)) { left = true; }
  int open(av1mi_ctx *c, uint32_t n_frames, bool mode_on, const char *mode_off, uintptr_t device_ptrs) {
    if (rc) { set_err(c, "invalid parameters"); return rc; }
    if (!mode_on) { set_err(c, "%s", mode_off); return AV1MI_E_INVALID_ARG; }
    if (device_ptrs & 15) { set_err(c, "device frames must be 16-byte aligned"); return AV1MI_E_INVALID_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    P = dev_params(r, n_frames, 1);
    left = false;
    return AV1MI_OK;
  }
};

// n caller frames on the device, as the encoder's source is.  tight: in the caller's layout - uploaded if they are on the host.  coded:
// at the coded size - edge-extended into a buffer of the pass's if that is not the signalled size, else `tight` - unless want_coded is
// off.  own_copy: `coded` is always a buffer of the pass's, which it may write - `own` - never the caller's memory.  All null after a
// failure (t.e).
struct PassFrames { const void *tight = nullptr, *coded = nullptr; void *own = nullptr; };
size_t coded_bytes(const Resolved &r, size_t n_frames) { return n_frames * r.cw * r.ch * 3 / 2 * (r.p.bit_depth > 8 ? 2 : 1); }
PassFrames coded_frames(PassBuffers &t, const Resolved &r, const void *frames, uint32_t n_frames, int on_device, bool own_copy = false, bool want_coded = true) {
  const size_t in_bytes = caller_bytes(r, n_frames);
  const bool make = want_coded && (r.padded || own_copy), direct = make && !r.padded;   // direct: the copy is made from the caller's memory
  PassFrames F;
  void *d_in = nullptr, *d_coded = nullptr;
  if (!on_device && !direct && t.alloc(d_in, in_bytes)) t.e = hipMemcpyAsync(d_in, frames, in_bytes, hipMemcpyHostToDevice, t.stream);
  if (make) t.alloc(d_coded, coded_bytes(r, n_frames));
  F.tight = direct ? d_coded : (on_device ? frames : d_in);
  if (t.ok() && direct) t.e = hipMemcpyAsync(d_coded, frames, in_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, t.stream);
  else if (t.ok() && make) t.e = av1mi_launch_pad(F.tight, d_coded, (int)r.p.width, (int)r.p.height, r.cw, r.ch, (int)r.p.bit_depth, (int)n_frames, 0, t.stream);
  if (want_coded) F.coded = make ? d_coded : F.tight;
  if (own_copy) F.own = d_coded;
  return t.ok() ? F : PassFrames();
}

// a result of the pass to host memory, where the caller asks for it
void to_host(PassBuffers &t, void *dst, const void *d_src, size_t bytes) {
  if (t.ok() && dst && bytes) t.e = hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, t.stream);
}

// a pass's result at the coded size, cropped to the caller's layout and copied to `out` - where the caller's frames are, host or device
void return_frames(PassBuffers &t, const Resolved &r, const void *d_coded, void *out, uint32_t n_frames, int frames_on_device) {
  const size_t in_bytes = caller_bytes(r, n_frames);
  void *d_crop = nullptr;
  if (r.padded && t.alloc(d_crop, in_bytes)) t.e = av1mi_launch_pad(d_coded, d_crop, (int)r.p.width, (int)r.p.height, r.cw, r.ch, (int)r.p.bit_depth, (int)n_frames, 1, t.stream);
  if (t.ok()) t.e = hipMemcpyAsync(out, r.padded ? d_crop : d_coded, in_bytes, frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, t.stream);
}

}  // namespace

extern "C" {

// The scene-cut pass works on the caller's tight layout with the frame before the first: it shares the passes' buffer owner and error
// mapping, not their frames at the coded size.
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
  PassBuffers t(s);
  // host input: stage [prev | frames] contiguously on the device (frame_bytes is a multiple of 32)
  uint8_t *d_stage = nullptr;
  unsigned long long *d_sad = nullptr;
  const uint8_t *d_frames, *d_prev = nullptr;
  if (t.alloc(d_sad, (size_t)n_frames * 8)) t.e = hipMemsetAsync(d_sad, 0, (size_t)n_frames * 8, s);
  if (t.ok() && !frames_on_device) {
    if (t.alloc(d_stage, (size_t)(n_frames + 1) * frame_bytes) && prev_frame) t.e = hipMemcpyAsync(d_stage, prev_frame, frame_bytes, hipMemcpyHostToDevice, s);
    if (t.ok()) t.e = hipMemcpyAsync(d_stage + frame_bytes, frames, (size_t)n_frames * frame_bytes, hipMemcpyHostToDevice, s);
    d_frames = d_stage + frame_bytes;
    d_prev = prev_frame ? d_stage : nullptr;
  } else {
    d_frames = (const uint8_t *)frames;
    d_prev = (const uint8_t *)prev_frame;
    if (((uintptr_t)d_frames | (uintptr_t)d_prev) & 15) { set_err(c, "device frames must be 16-byte aligned"); return AV1MI_E_INVALID_ARG; }
  }
  std::vector<unsigned long long> sad(n_frames, 0);
  if (t.ok()) t.e = av1mi_launch_luma_sad(&P, d_frames, d_prev, d_sad, s);
  if (t.ok()) t.e = hipMemcpyAsync(sad.data(), d_sad, (size_t)n_frames * 8, hipMemcpyDeviceToHost, s);
  rc = t.finish(c, "scene-cut");
  if (rc) return rc;
  const uint64_t luma = (uint64_t)r.p.width * r.p.height;
  for (uint32_t f = 0; f < n_frames; f++) {
    const int has_prev = f > 0 || prev_frame != nullptr;
    const int cut = scene_rule_step(state, has_prev, sad[f], luma, (int)r.p.bit_depth, min_scene_len ? min_scene_len : 1);
    if (is_cut) is_cut[f] = (uint8_t)cut;
    if (sad_out) sad_out[f] = sad[f];
  }
  return AV1MI_OK;
}

}  // extern "C"

namespace {
// The temporal-dependency analysis of a stand-alone pass: its five buffers, the flow cleared, and the launches (av1mi_launch_tpl) on
// `src`, n frames at the coded size taken as one chunk.  What failed is in t.e.
struct TplBuffers {
  uint32_t *intra = nullptr, *inter = nullptr, *key = nullptr;
  unsigned long long *flow = nullptr;
  uint16_t *beta = nullptr;
  size_t n_blk = 0, n_flow = 0;
  const unsigned long long *beta_sum() const { return flow + n_flow - 1; }
};
void run_tpl(PassBuffers &t, const Resolved &r, const Av1miDevParams &P, const void *src, uint32_t n_frames, TplBuffers &b) {
  b.n_flow = av1mi_tpl_flow_entries(r.cw, r.ch, (int)n_frames);
  b.n_blk = b.n_flow - 1;
  t.alloc(b.intra, b.n_blk * sizeof(uint32_t));
  t.alloc(b.inter, b.n_blk * sizeof(uint32_t));
  t.alloc(b.key, b.n_blk * sizeof(uint32_t));
  t.alloc(b.flow, b.n_flow * sizeof(unsigned long long));
  t.alloc(b.beta, (size_t)n_frames * r.sb_cols * r.sb_rows * sizeof(uint16_t));
  if (t.ok()) t.e = hipMemsetAsync(b.flow, 0, b.n_flow * sizeof(unsigned long long), t.stream);
  if (t.ok()) t.e = av1mi_launch_tpl(&P, src, b.intra, b.inter, b.key, b.flow, b.beta, t.stream);
}
// ... and the frame term's sums behind it (av1mi_launch_tpl_frames), in a block of the pass's
Av1miFqBlock run_fq(PassBuffers &t, const Av1miDevParams &P, uint32_t n_frames, const TplBuffers &b) {
  uint8_t *d = nullptr;
  t.alloc(d, av1mi_fq_bytes(n_frames));
  const Av1miFqBlock fq = av1mi_fq_split(d, n_frames);
  if (t.ok()) t.e = av1mi_launch_tpl_frames(&P, b.intra, b.flow, b.beta, fq, t.stream);
  return fq;
}
}  // namespace

extern "C" {

// The adaptive quantisation's decision alone: the same launches the encoder runs on a chunk's source (av1mi_launch_tpl with a temporal
// strength, av1mi_launch_aq), on buffers of the call's own.
int av1mi_aq_qindex(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, uint8_t *qindex) {
  if (!c || !frames || !qindex || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  const Resolved &r = t.r; const Av1miDevParams &P = t.P; hipStream_t s = t.stream;
  const size_t n_map = (size_t)n_frames * r.sb_cols * r.sb_rows;
  if (!t.rc && !qmap_on(r)) { memset(qindex, r.qidx, n_map); return AV1MI_OK; }   // every superblock at the chunk's index: nothing looks at the frames or their alignment
  if (const int rc = t.open(c, n_frames, true, nullptr, frames_on_device ? (uintptr_t)frames : 0)) return rc;
  uint16_t *d_act = nullptr;
  uint8_t *d_map = nullptr;
  TplBuffers tpl;
  Av1miFqMap fq = {};
  t.alloc(d_act, n_map * sizeof(uint16_t));
  t.alloc(d_map, n_map);
  const void *src = coded_frames(t, r, frames, n_frames, frames_on_device).coded;   // the rule reads the coded size
  if (r.tpl || r.fq) run_tpl(t, r, P, src, n_frames, tpl);
  if (r.fq) { fq.strength = r.fq; fq.fq = run_fq(t, P, n_frames, tpl); }   // the combined map: the frames' steps included
  if (t.ok()) t.e = av1mi_launch_aq(&P, src, d_act, d_map, r.aq, tpl.beta, r.tpl ? tpl.beta_sum() : nullptr, r.tpl, &fq, s);
  if (t.ok()) t.e = hipMemcpyAsync(qindex, d_map, n_map, hipMemcpyDeviceToHost, s);
  return t.finish(c, "adaptive-quantisation");
}

// The frame term's decision alone: the encoder's launches (av1mi_launch_tpl, av1mi_launch_tpl_frames, aq_map_kernel's frame step) on the
// frames it is given, on buffers of the call's own and without a header to write into.
int av1mi_tpl_frame_q(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, uint64_t *intra_sum,
                      uint64_t *dep_sum, uint16_t *beta, uint32_t *mean_beta, uint8_t *frame_q) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  if (const int rc = t.open(c, n_frames, t.r.fq, "the frame strength is 0", frames_on_device ? (uintptr_t)frames : 0)) return rc;
  TplBuffers b;
  Av1miFqMap fq = {};
  uint8_t *d_map = nullptr;
  t.alloc(d_map, (size_t)n_frames * t.r.sb_cols * t.r.sb_rows);
  const void *src = coded_frames(t, t.r, frames, n_frames, frames_on_device).coded;
  if (t.ok()) run_tpl(t, t.r, t.P, src, n_frames, b);
  fq.strength = t.r.fq;
  fq.fq = run_fq(t, t.P, n_frames, b);
  if (t.ok()) t.e = av1mi_launch_aq(&t.P, src, nullptr, d_map, 0, b.beta, nullptr, 0, &fq, t.stream);   // (the map, all q_f, is not reported)
  std::vector<uint16_t> bf(n_frames, 0);
  to_host(t, intra_sum, fq.fq.intra_sum, (size_t)n_frames * 8);
  to_host(t, dep_sum, fq.fq.dep_sum, (size_t)n_frames * 8);
  to_host(t, bf.data(), fq.fq.beta, (size_t)n_frames * 2);
  to_host(t, frame_q, fq.fq.frame_q, n_frames);
  const int rc = t.finish(c, "frame-quantiser");   // (drains the stream: `bf` has arrived)
  if (rc != AV1MI_OK) return rc;
  uint64_t sum = 0;
  for (uint32_t f = 0; f < n_frames; f++) sum += bf[f];
  if (beta) memcpy(beta, bf.data(), (size_t)n_frames * 2);
  if (mean_beta) *mean_beta = (uint32_t)av1mi_fq_mean(sum, n_frames);
  return AV1MI_OK;
}

// One chunk against another on the device (quality_kernel.hip), both in the callers' tight layout as the scene-cut pass takes its frames.
int av1mi_quality(av1mi_ctx *c, const av1mi_params *params, const void *ref, const void *test, uint32_t n_frames, int frames_on_device,
                  av1mi_plane_quality *out, int32_t *window_map) {
  if (!c || !params || !ref || !test || !out || n_frames == 0) return AV1MI_E_INVALID_ARG;
  av1mi_params size;   // only the size and the depth matter: whatever else the caller's parameters say is not looked at
  av1mi_default_params(&size, params->width, params->height, params->bit_depth);
  Pass t(c, &size);
  if (const int rc = t.open(c, n_frames, true, nullptr, frames_on_device ? (uintptr_t)ref | (uintptr_t)test : 0)) return rc;
  const Resolved &r = t.r;
  const Av1miQualityGeom G = av1mi_quality_geom((int)r.p.width, (int)r.p.height, (int)r.p.width, (int)r.p.height, (int)r.p.bit_depth);
  const size_t n_sums = (size_t)n_frames * 3 * 2, n_map = (size_t)n_frames * G.map_frame;
  unsigned long long *d_sums = nullptr;
  int32_t *d_map = nullptr;
  if (t.alloc(d_sums, n_sums * sizeof(unsigned long long))) t.e = hipMemsetAsync(d_sums, 0, n_sums * sizeof(unsigned long long), t.stream);
  if (window_map) t.alloc(d_map, n_map * sizeof(int32_t));
  const void *a = coded_frames(t, r, ref, n_frames, frames_on_device, false, false).tight;
  const void *b = coded_frames(t, r, test, n_frames, frames_on_device, false, false).tight;
  if (t.ok()) t.e = av1mi_launch_quality(&G, a, b, (int)n_frames, d_sums, d_map, t.stream);
  std::vector<unsigned long long> sums(n_sums, 0);
  to_host(t, sums.data(), d_sums, n_sums * sizeof(unsigned long long));
  to_host(t, window_map, d_map, n_map * sizeof(int32_t));
  const int rc = t.finish(c, "quality");   // (drains the stream: `sums` has arrived)
  if (rc != AV1MI_OK) return rc;
  for (size_t i = 0; i < (size_t)n_frames * 3; i++) out[i] = plane_quality(&sums[i * 2], G, (int)(i % 3));
  return AV1MI_OK;
}

int av1mi_ctx_set_quality(av1mi_ctx *c, uint32_t on) {
  if (!c) return AV1MI_E_INVALID_ARG;
  c->quality = on != 0;
  return AV1MI_OK;
}

// The quality of the context's last chunk: what download_chunk kept, zeros for a chunk encoded with the switch off.
int av1mi_quality_result(const av1mi_ctx *c, uint32_t n_frames, av1mi_plane_quality *out) {
  if (!c || !out || !c->last.n_frames || n_frames != c->last.n_frames) return AV1MI_E_INVALID_ARG;
  memcpy(out, c->last.quality.data(), (size_t)n_frames * 3 * sizeof(av1mi_plane_quality));
  return AV1MI_OK;
}

// What the last chunk's frame headers carry: the rule's parameter set of its mode, table and coefficients.
int av1mi_film_grain_params_result(const av1mi_ctx *c, av1mi_grain_params *g) {
  if (!c || !g || !c->last.n_frames || !c->last.film_grain) return AV1MI_E_INVALID_ARG;
  av1mi_fgs_header_params((int)c->last.film_grain, c->last.fg_estimate, c->last.fg_ar_lag, c->last.fg_table, c->last.fg_ar_coeffs, g);
  return AV1MI_OK;
}

int av1mi_ctx_set_displayed_quality(av1mi_ctx *c, uint32_t on) {
  if (!c) return AV1MI_E_INVALID_ARG;
  c->displayed = on != 0;
  return AV1MI_OK;
}

// The displayed picture's quality of the context's last chunk: what download_chunk kept, zeros with the switch off or without film grain.
int av1mi_displayed_quality_result(const av1mi_ctx *c, uint32_t n_frames, av1mi_plane_quality *out) {
  if (!c || !out || !c->last.n_frames || n_frames != c->last.n_frames) return AV1MI_E_INVALID_ARG;
  memcpy(out, c->last.displayed.data(), (size_t)n_frames * 3 * sizeof(av1mi_plane_quality));
  return AV1MI_OK;
}

uint32_t av1mi_grain_params_size(void) { return (uint32_t)sizeof(av1mi_grain_params); }

// What a decoder adds to the frames (fg_synth_kernel.hip), in the callers' tight layout as the quality pass takes its frames: the
// templates' launch and the frames' on buffers of the call's own.
int av1mi_film_grain_synth(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                           const av1mi_grain_params *g, const uint16_t *seeds, void *out) {
  if (!c || !params || !frames || !g || !out || out == frames || n_frames == 0 || n_frames > 65535) return AV1MI_E_INVALID_ARG;
  if (!av1mi_fgs_params_valid(*g)) { set_err(c, "invalid film-grain parameters"); return AV1MI_E_INVALID_ARG; }
  av1mi_params size;   // only the size and the depth matter, and the first frame's number for the seeds
  av1mi_default_params(&size, params->width, params->height, params->bit_depth);
  Pass t(c, &size);
  if (const int rc = t.open(c, n_frames, true, nullptr, frames_on_device ? (uintptr_t)frames | (uintptr_t)out : 0)) return rc;
  const Resolved &r = t.r;
  const size_t bytes = caller_bytes(r, n_frames);
  if (!av1mi_fgs_any_plane_on(*g)) {   // no scaling function: the frames as they are
    if (frames_on_device) t.e = hipMemcpyAsync(out, frames, bytes, hipMemcpyDeviceToDevice, t.stream);
    else memcpy(out, frames, bytes);
    return t.finish(c, "film-grain synthesis");
  }
  const int w = (int)r.p.width, h = (int)r.p.height;
  const Av1miQualityGeom G = av1mi_quality_geom(w, h, w, h, (int)r.p.bit_depth);
  uint8_t *d_block = nullptr;
  uint16_t *d_seeds = nullptr;
  void *d_out = frames_on_device ? out : nullptr;
  t.alloc(d_block, av1mi_fgs_bytes(n_frames, (size_t)av1mi_fgs_stripes(h) * av1mi_fgs_blocks(w)));
  if (seeds && t.alloc(d_seeds, (size_t)n_frames * sizeof(uint16_t))) t.e = hipMemcpyAsync(d_seeds, seeds, (size_t)n_frames * sizeof(uint16_t), hipMemcpyHostToDevice, t.stream);
  if (!frames_on_device) t.alloc(d_out, bytes);
  const void *in = coded_frames(t, r, frames, n_frames, frames_on_device, false, false).tight;
  const Av1miFgsBlock B = av1mi_fgs_split(d_block, n_frames);
  if (t.ok()) t.e = hipMemcpyAsync(B.g, g, sizeof(*g), hipMemcpyHostToDevice, t.stream);
  if (t.ok()) t.e = av1mi_launch_fg_synth_templates((int)r.p.bit_depth, w, h, (int)n_frames, d_seeds, params->first_frame, B, t.stream);
  if (t.ok()) t.e = av1mi_launch_fg_synth_apply(&G, &G, in, d_out, (int)n_frames, B, t.stream);
  if (!frames_on_device) to_host(t, out, d_out, bytes);
  return t.finish(c, "film-grain synthesis");
}

// The frames' base_q_idx and betaF of the context's last chunk: what download_chunk kept.
int av1mi_frame_q_result(const av1mi_ctx *c, uint32_t n_frames, uint8_t *frame_q, uint16_t *beta) {
  if (!c || !c->last.n_frames || n_frames != c->last.n_frames) return AV1MI_E_INVALID_ARG;
  if (frame_q) memcpy(frame_q, c->last.frame_q.data(), n_frames);
  if (beta) memcpy(beta, c->last.frame_beta.data(), (size_t)n_frames * sizeof(uint16_t));
  return AV1MI_OK;
}

// The temporal-dependency analysis alone: the launches the encoder runs on a chunk's source (av1mi_launch_tpl), on buffers of the call's own.
int av1mi_tpl_analysis(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, uint32_t *intra,
                       uint32_t *inter, uint32_t *key, uint64_t *flow, uint16_t *beta, uint32_t *mean_beta) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  if (const int rc = t.open(c, n_frames, t.r.tpl, "the temporal strength is 0", frames_on_device ? (uintptr_t)frames : 0)) return rc;
  TplBuffers b;
  const void *src = coded_frames(t, t.r, frames, n_frames, frames_on_device).coded;
  if (t.ok()) run_tpl(t, t.r, t.P, src, n_frames, b);
  unsigned long long sum = 0;
  const size_t n_sb = (size_t)n_frames * t.r.sb_cols * t.r.sb_rows;
  to_host(t, intra, b.intra, b.n_blk * sizeof(uint32_t));
  to_host(t, inter, b.inter, b.n_blk * sizeof(uint32_t));
  to_host(t, key, b.key, b.n_blk * sizeof(uint32_t));
  to_host(t, flow, b.flow, b.n_blk * sizeof(unsigned long long));
  to_host(t, beta, b.beta, n_sb * sizeof(uint16_t));
  if (t.ok() && mean_beta) to_host(t, &sum, b.beta_sum(), sizeof(sum));
  const int rc = t.finish(c, "temporal-dependency");   // (drains the stream: `sum` has arrived)
  if (rc == AV1MI_OK && mean_beta) *mean_beta = (uint32_t)av1mi_tpl_mean_beta(sum, n_sb);
  return rc;
}

// The three film-grain passes alone run launch_grain_passes, as prepare_chunk does, on blocks and buffers of the call's own and without
// a header to write into.
int av1mi_film_grain_estimate(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, uint8_t *table,
                              uint32_t *counts, uint8_t *blocks) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  if (const int rc = t.open(c, n_frames, t.r.fg_estimate, "film_grain does not ask for the estimate", frames_on_device ? (uintptr_t)frames : 0)) return rc;
  const size_t n_blk = fg_records(t.r, n_frames);
  uint8_t *d_fg = nullptr;
  t.alloc(d_fg, av1mi_fg_bytes(n_blk));
  const PassFrames F = coded_frames(t, t.r, frames, n_frames, frames_on_device);
  if (t.ok()) t.e = launch_grain_passes(t.P, t.r, nullptr, F.coded, d_fg, nullptr, nullptr, nullptr, Av1miFgBits{}, t.stream);
  const Av1miFgBlock fg = av1mi_fg_split(d_fg);
  to_host(t, table, fg.table, AV1MI_FG_TABLE);
  to_host(t, counts, fg.counts, AV1MI_FG_TABLE * sizeof(uint32_t));
  to_host(t, blocks, fg.blocks, n_blk * sizeof(uint32_t));
  return t.finish(c, "film-grain");
}

}  // extern "C"

namespace {
// ... the denoiser: the estimate unless the caller gives the table; the result cropped to the caller's layout.  With the temporal term
// (the field's bits 14 and 15) the search's keys as well, unless the caller gives them - use_mv, n_frames * 4 * blocks entries on the host:
// the indexes as they are, all-ones for "no neighbour", an index no vector of the range has refused, and the entries of neighbours frame f
// cannot have at the span made all-ones; mv: the keys the filter ran with.  need_temporal: the field must carry the term
int denoise_pass(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, const uint8_t *use_table,
                 const uint32_t *use_mv, void *out, uint8_t *table, uint32_t *mv, bool need_temporal) {
  Pass t(c, params);
  const uintptr_t device_ptrs = frames_on_device ? (uintptr_t)frames | (uintptr_t)out : 0;
  const bool mode = !t.rc && t.r.fg_denoise && (!need_temporal || t.r.fg_denoise_span);
  const int span = mode ? t.r.fg_denoise_span : 0;
  const size_t n_mv = span ? fgd_mv_entries(t.r, n_frames) : 0, nb = n_mv / n_frames / AV1MI_FGD_SLOTS;
  std::vector<uint32_t> given;
  if (span && use_mv) {   // (checked like the other arguments, before a device is touched)
    const uint32_t nc = 2 * t.r.p.me_range + 1;
    given.assign(use_mv, use_mv + n_mv);
    for (size_t i = 0; i < n_mv; i++) {
      if (!av1mi_fgd_slot_exists((int)(i / (AV1MI_FGD_SLOTS * nb)), (int)(i / nb % AV1MI_FGD_SLOTS), span, (int)n_frames)) given[i] = AV1MI_FGD_NONE;
      else if (given[i] != AV1MI_FGD_NONE && (given[i] & 0x7FFu) >= nc * nc) {
        set_err(c, "use_mv[%zu]: index %u is no vector of the range", i, given[i] & 0x7FFu);
        return AV1MI_E_INVALID_ARG;
      }
    }
  }
  if (const int rc = t.open(c, n_frames, mode, need_temporal ? "film_grain does not ask for the denoiser's temporal term" : "film_grain does not ask for the denoiser", device_ptrs))
    return rc;
  uint8_t *d_fg = nullptr;
  void *d_den = nullptr;
  uint32_t *d_mv = nullptr;
  t.alloc(d_fg, av1mi_fg_bytes(fg_records(t.r, n_frames)));
  if (out) t.alloc(d_den, coded_bytes(t.r, n_frames));
  if (span) t.alloc(d_mv, n_mv * sizeof(uint32_t));
  if (t.ok() && span && use_mv) t.e = hipMemcpyAsync(d_mv, given.data(), n_mv * sizeof(uint32_t), hipMemcpyHostToDevice, t.stream);   // (`given` outlives the pass: finish() drains)
  // (the estimate and the search read the coded size)
  const PassFrames F = coded_frames(t, t.r, frames, n_frames, frames_on_device, false, !use_table || (span && !use_mv));
  if (t.ok() && use_table) t.e = hipMemcpyAsync(d_fg, use_table, AV1MI_FG_TABLE, hipMemcpyHostToDevice, t.stream);
  if (t.ok()) t.e = launch_grain_passes(t.P, t.r, F.tight, F.coded, d_fg, nullptr, d_den, nullptr, Av1miFgBits{}, t.stream, d_mv, use_mv != nullptr, !use_table);
  if (t.ok() && out) return_frames(t, t.r, d_den, out, n_frames, frames_on_device);
  to_host(t, table, d_fg, AV1MI_FG_TABLE);
  to_host(t, mv, d_mv, n_mv * sizeof(uint32_t));
  return t.finish(c, "film-grain denoise");
}
}  // namespace

extern "C" {

int av1mi_film_grain_denoise(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, const uint8_t *use_table,
                             void *out, uint8_t *table) {
  if (!c || !frames || !out || n_frames == 0) return AV1MI_E_INVALID_ARG;
  return denoise_pass(c, params, frames, n_frames, frames_on_device, use_table, nullptr, out, table, nullptr, false);
}

// ... with the temporal term, its keys reported or given
int av1mi_film_grain_denoise_temporal(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                                      const uint8_t *use_table, const uint32_t *use_mv, void *out, uint8_t *table, uint32_t *mv) {
  if (!c || !frames || (!out && !mv) || n_frames == 0) return AV1MI_E_INVALID_ARG;
  return denoise_pass(c, params, frames, n_frames, frames_on_device, use_table, use_mv, out, table, mv, true);
}

// ... the autoregressive fit, behind the estimate
int av1mi_film_grain_ar_estimate(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, int8_t *coeffs,
                                 uint8_t *table, uint8_t *sigma_table, uint32_t *gain, uint32_t *flat_blocks, int64_t *sums) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  if (const int rc = t.open(c, n_frames, t.r.fg_ar_lag, "film_grain does not ask for the autoregressive fit", frames_on_device ? (uintptr_t)frames : 0)) return rc;
  uint8_t *d_fg = nullptr, *d_ar = nullptr;
  t.alloc(d_fg, av1mi_fg_bytes(fg_records(t.r, n_frames)));
  t.alloc(d_ar, av1mi_fgar_bytes());
  const PassFrames F = coded_frames(t, t.r, frames, n_frames, frames_on_device);
  if (t.ok()) t.e = launch_grain_passes(t.P, t.r, nullptr, F.coded, d_fg, d_ar, nullptr, nullptr, Av1miFgBits{}, t.stream);
  const Av1miFgArBlock ar = av1mi_fgar_split(d_ar);
  to_host(t, coeffs, ar.coeffs, 3 * AV1MI_FGAR_COEFFS);
  to_host(t, table, ar.table, AV1MI_FG_TABLE);
  to_host(t, sigma_table, ar.sigma, AV1MI_FG_TABLE);
  to_host(t, gain, ar.gain, 3 * sizeof(uint32_t));
  to_host(t, flat_blocks, ar.flat, 3 * sizeof(uint32_t));
  to_host(t, sums, ar.sums, 3 * AV1MI_FGAR_SUMS * sizeof(int64_t));
  return t.finish(c, "film-grain autoregressive fit");
}

// The autoregressive fit of the context's last chunk: what download_chunk kept, zeros and gains of 256 for a chunk without a lag.
int av1mi_film_grain_ar_result(const av1mi_ctx *c, int8_t *coeffs, uint8_t *sigma_table, uint32_t *gain) {
  if (!c || !c->last.n_frames) return AV1MI_E_INVALID_ARG;
  if (coeffs) memcpy(coeffs, c->last.fg_ar_coeffs, sizeof(c->last.fg_ar_coeffs));
  if (sigma_table) memcpy(sigma_table, c->last.fg_sigma_table, sizeof(c->last.fg_sigma_table));
  if (gain) memcpy(gain, c->last.fg_ar_gain, sizeof(c->last.fg_ar_gain));
  return AV1MI_OK;
}

// The film-grain table of the context's last chunk: what download_chunk kept, zeros for a chunk without the estimate.
int av1mi_film_grain_result(const av1mi_ctx *c, uint8_t *table) {
  if (!c || !table || !c->last.n_frames) return AV1MI_E_INVALID_ARG;
  memcpy(table, c->last.fg_table, sizeof(c->last.fg_table));
  return AV1MI_OK;
}

// The temporal filter alone: the launch the encoder runs on a chunk's source (av1mi_launch_temporal_filter), on buffers of the call's own.
int av1mi_temporal_filter(av1mi_ctx *c, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device, void *out,
                          uint32_t *mv) {
  if (!c || !frames || n_frames == 0) return AV1MI_E_INVALID_ARG;
  Pass t(c, params);
  if (const int rc = t.open(c, n_frames, true, nullptr, 0)) return rc;   // (no mode, and no alignment to ask for: the filter works on a copy of the pass's)
  const size_t n_mv = tf_mv_entries(t.r, n_frames);
  uint32_t *d_mv = nullptr;
  if (n_mv) t.alloc(d_mv, n_mv * sizeof(uint32_t));
  void *d_coded = coded_frames(t, t.r, frames, n_frames, frames_on_device, true).own;   // the filter works in place at the coded size
  if (t.ok() && n_mv) t.e = av1mi_launch_temporal_filter(&t.P, d_coded, d_mv, t.r.tf_frames, t.r.tf_strength, t.stream);
  if (t.ok() && out) return_frames(t, t.r, d_coded, out, n_frames, frames_on_device);
  to_host(t, mv, d_mv, n_mv * sizeof(uint32_t));
  return t.finish(c, "temporal-filter");
}

// The levels the context's last chunk was deblocked with and, with the level search, the candidates' errors: what download_chunk kept.
int av1mi_lf_search_result(const av1mi_ctx *c, uint32_t n_frames, uint8_t *levels, uint64_t *err) {
  if (!c || !levels || n_frames == 0 || c->last.n_frames != n_frames) return AV1MI_E_INVALID_ARG;
  memcpy(levels, c->last.lf_levels.data(), c->last.lf_levels.size());
  if (err) memcpy(err, c->last.lf_errs.data(), c->last.lf_errs.size() * sizeof(unsigned long long));
  return AV1MI_OK;
}

uint32_t av1mi_lr_fit_units(const av1mi_ctx *c) { return c ? c->last.fit_plane_units : 0; }
// The self-guided fit of the context's last chunk: what download_chunk fetched, zeros for a chunk without the fit.
int av1mi_lr_fit_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *units, uint64_t *err) {
  if (!c || !units || n_frames == 0 || c->last.n_frames != n_frames) return AV1MI_E_INVALID_ARG;
  const size_t n = c->last.fit_units;
  if (c->last.fit_on) {
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
  if (!c || !order || !classes || !c->last.n_frames || n != c->last.sym_tiles || n == 0) return AV1MI_E_INVALID_ARG;
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
uint32_t av1mi_sym_order_tiles(const av1mi_ctx *c) { return c && c->last.n_frames ? c->last.sym_tiles : 0; }

// The partition of the last chunk's frames and the integer search's keys, as they still stand on the device (the context's next chunk
// overwrites them), fetched here - a diagnostic like av1mi_sym_order_result.
uint32_t av1mi_inter_partition_units(const av1mi_ctx *c) { return c && c->last.n_frames && c->last.pi_frames ? c->last.pi_units : 0; }
int av1mi_inter_partition_result(const av1mi_ctx *c, uint32_t n_frames, uint32_t *masks, uint64_t *keys) {
  if (!c || !masks || !keys || n_frames == 0 || !c->last.n_frames || c->last.pi_frames != n_frames) return AV1MI_E_INVALID_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return AV1MI_E_HIP;
  if (hipMemcpy(masks, c->ws.d_part, (size_t)n_frames * c->last.pi_sbs * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  // (the keys are the node-mode search's: a chunk without it - partition_search = 1, or no inter frame - reports zeros)
  if (!c->last.pi_keys) memset(keys, 0, (size_t)n_frames * c->last.pi_units * sizeof(uint64_t));
  else if (hipMemcpy(keys, c->ws.d_me, (size_t)n_frames * c->last.pi_units * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  return AV1MI_OK;
}

uint32_t av1mi_lr_wiener_fit_units(const av1mi_ctx *c) { return c ? c->last.fit_plane_units : 0; }
// The Wiener fit of the context's last chunk, likewise.
int av1mi_lr_wiener_fit_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *units, uint64_t *err) {
  if (!c || !units || n_frames == 0 || c->last.n_frames != n_frames) return AV1MI_E_INVALID_ARG;
  const size_t n = c->last.fit_units;
  if (c->last.wfit_on) {
    const Av1miLrWfit H = av1mi_lr_wfit_split(c->ws.h_wfit, n);   // the fetched head of the block
    memcpy(units, H.rec, n * 8);
    if (err) memcpy(err, H.err, n * 8);
  } else {
    memset(units, 0, n * 8);
    if (err) memset(err, 0, n * 8);
  }
  return AV1MI_OK;
}

uint32_t av1mi_lr_rd_units(const av1mi_ctx *c) { return c ? c->last.fit_plane_units : 0; }
// The final restoration decisions of the context's last chunk: the choices as they still stand on the device (the context's next chunk
// overwrites them), fetched here - a diagnostic like av1mi_sym_order_result - and their B16 from the fits' records, which arrived with
// the chunk.
int av1mi_lr_rd_result(const av1mi_ctx *c, uint32_t n_frames, int8_t *choice, uint32_t *bits16, uint64_t *lambda) {
  if (!c || !choice || n_frames == 0 || c->last.n_frames != n_frames) return AV1MI_E_INVALID_ARG;
  const Av1miDevParams &P = c->P;
  const size_t n = c->last.fit_units, per = c->last.fit_plane_units;
  memset(choice, 0, n);
  if (bits16) memset(bits16, 0, n * sizeof(uint32_t));
  if (lambda) *lambda = P.enable_lr ? P.lr_lambda : 0;
  if (!P.enable_lr) return AV1MI_OK;
  const int planes = P.lr_chroma ? 3 : 1, sw = P.enable_lr == 2;
  std::vector<uint8_t> dev((size_t)n_frames * planes * per);   // [frame][restored plane][unit]
  if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(dev.data(), c->ws.d_lrc, dev.size(), hipMemcpyDeviceToHost) != hipSuccess) return AV1MI_E_HIP;
  const Av1miLrFit G = c->last.fit_on ? av1mi_lr_fit_split(c->ws.h_fit, n, 0) : Av1miLrFit{};
  const Av1miLrWfit W = c->last.wfit_on ? av1mi_lr_wfit_split(c->ws.h_wfit, n) : Av1miLrWfit{};
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
}  // extern "C"
