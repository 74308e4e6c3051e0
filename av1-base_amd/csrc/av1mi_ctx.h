// av1mi_ctx.h - the encoder context and what it owns: the device workspace, the streams and events, the error text and the record
// of its last chunk.  av1mi_ctx.cpp keeps them (and runs the stand-alone passes); av1mi_host.cpp encodes one chunk on them.
#ifndef AV1MI_CTX_H
#define AV1MI_CTX_H
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "av1mi_syntax.h"
#include "av1mi_launch.h"
#include "fg_rule.h"

namespace av1mi {

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
  // the temporal-dependency analysis (tpl_kernel.hip), on first use: per [frame][16x16 block] I, C and the search's key, the flow A with
  // the chunk's sum of beta behind it (av1mi_tpl_flow_entries: one fill clears both), and beta per [frame][superblock]
  uint32_t *d_tpl_intra = nullptr, *d_tpl_inter = nullptr, *d_tpl_key = nullptr;
  unsigned long long *d_tpl_flow = nullptr;
  uint16_t *d_tpl_beta = nullptr;
  // the frame term (cq_level bits 20-22), on first use: its block (av1mi_fq_split) - per frame OF, PF, the sum of beta, betaF and q_f - and
  // where one copy lands it
  uint8_t *d_fq = nullptr, *h_fq = nullptr;
  // the film-grain estimate (fg_kernel.hip), on first use: its block (av1mi_fg_split); h_fg: where one copy lands its head
  uint8_t *d_fg = nullptr, *h_fg = nullptr;
  // the grain's autoregressive fit (fg_ar_kernel.hip), on first use: its block (av1mi_fgar_split), and where one copy lands its head
  uint8_t *d_fg_ar = nullptr, *h_fg_ar = nullptr;
  uint32_t *d_fgd_mv = nullptr;            // the film-grain denoiser's temporal term: the search's keys per [frame][slot][16x16 block] (fg_denoise_rule.h)
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
  // the quality pass inside the encoder (av1mi_ctx_set_quality), on first use: per [frame][plane] the squared error and the sum of
  // window values (av1mi_launch_quality), and where one copy lands them
  unsigned long long *d_quality = nullptr, *h_quality = nullptr;
  // the displayed picture's quality (av1mi_ctx_set_displayed_quality), on first use with film grain: the synthesis' block
  // (av1mi_fgs_split), the final frames with their grain in the caller's tight layout, the quality pass's sums of those against the
  // caller's frames, and where one copy lands them
  uint8_t *d_fgs = nullptr;
  void *d_disp = nullptr;
  unsigned long long *d_disp_quality = nullptr, *h_disp_quality = nullptr;
  uint8_t *h_out = nullptr;            // host staging (pinned), for when the caller's buffer cannot be page-locked
  // Page-locked host side of the small transfers.  The chunk constants - header blob, default CDFs, parameters - are the same for
  // every chunk of a job: h_hdr / h_cdf / h_params hold what d_hdr / d_cdf / d_params hold, and prepare_chunk uploads only what differs.
  uint8_t *h_hdr = nullptr; uint16_t *h_cdf = nullptr; Av1miDevParams *h_params = nullptr;
  size_t hdr_bytes = 0;                // bytes of h_hdr that d_hdr is known to hold; 0: unknown (the strength search writes into d_hdr)
  int cdf_qidx = -1;                   // the quantiser index d_cdf was made for (the blob depends on nothing else); -1: none; AV1MI_CDF_ALL: the
                                       // four q contexts' blobs one after the other (the frame term)
  int cdf_bs_log2 = -1;                // ... and the leaf size its compact image behind the blob was made for
  int params_on_device = 0;            // d_params holds the first so many blocks of h_params (1, AV1MI_AQ_SLOTS with adaptive quantisation, AV1MI_FQ_SLOTS with the frame term)
  Av1miChunkRecord *h_record = nullptr; unsigned long long *h_sse = nullptr;   // d_record and d_sse land here
  size_t out_cap = 0, me64_bytes = 0, nodes_bytes = 0, h_out_cap = 0, tf_mv_bytes = 0, fgd_mv_bytes = 0;   // bytes of d_out, d_me64, d_nodes, h_out, d_tf_mv, d_fgd_mv
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

// What a context remembers of its last chunk for the *_result, *_units and *_tiles entry points: filled once the chunk has succeeded
// (run_chunk), reset when the next one starts.
struct LastChunk {
  uint32_t n_frames = 0;   // 0: no chunk yet, or the last one failed
  // its deblocking levels (4 per frame) and level-search errors (48 per frame; zeros without the search): av1mi_lf_search_result
  std::vector<uint8_t> lf_levels;
  std::vector<unsigned long long> lf_errs;
  // its self-guided fit (av1mi_lr_fit_result): the units of its frames over three planes, and whether the fit ran - the errors and
  // records are then the head of ws.h_fit
  size_t fit_units = 0;
  uint32_t fit_plane_units = 0;   // the units of one plane of one frame (av1mi_lr_fit_units)
  bool fit_on = false;
  bool wfit_on = false;           // ... and its Wiener fit (av1mi_lr_wiener_fit_result): the head of ws.h_wfit
  uint32_t sym_tiles = 0;         // the tiles of its weight-ordered table (av1mi_sym_order_result); 0: natural order
  bool pi_keys = false;           // it was partitioned from the search's node costs: its search keys are reported too
  uint32_t pi_frames = 0, pi_units = 0, pi_sbs = 0;   // with a partition map: frames (else 0), 8x8 units and superblocks per frame (av1mi_inter_partition_result)
  uint8_t fg_table[24] = {};      // the film-grain table its headers carry (av1mi_film_grain_result); zeros without the estimate
  // its autoregressive fit (av1mi_film_grain_ar_result): coefficients, the table before the gains, the gains; zeros and 256 without a lag
  int8_t fg_ar_coeffs[3 * 25] = {};
  uint8_t fg_sigma_table[24] = {};
  uint32_t fg_ar_gain[3] = { 256, 256, 256 };
  // its frames' base_q_idx and betaF (av1mi_frame_q_result): the chunk's index and zeros without the frame term
  std::vector<uint8_t> frame_q;
  std::vector<uint16_t> frame_beta;
  // its quality per [frame][plane] (av1mi_quality_result): zeros for a chunk encoded with the switch off
  std::vector<av1mi_plane_quality> quality;
  // the displayed picture's per [frame][plane] (av1mi_displayed_quality_result): zeros with the switch off or without film grain
  std::vector<av1mi_plane_quality> displayed;
  // what its headers' film_grain_params were made of (av1mi_film_grain_params_result): N (0: none), estimated, the lag
  uint32_t film_grain = 0;
  bool fg_estimate = false;
  int fg_ar_lag = 0;
};
#define AV1MI_CDF_ALL 256
// the records of the film-grain estimate over n_frames frames: the whole 16x16 blocks of the signalled size
inline size_t fg_records(const Resolved &r, size_t n_frames) { return n_frames * av1mi_fg_blocks((int)r.p.width) * av1mi_fg_blocks((int)r.p.height); }
// The grain passes `r` asks for, in the encoder's order on stream s: the estimate on `coded` - the caller's frames on the device at the
// coded size - into the estimate's block d_fg; the autoregressive fit on the same frames into the fit's block d_fg_ar; the denoiser from
// `tight`, the same frames in the caller's layout, by d_fg's table into `out` at the coded size.  A pass whose frames or block are null is
// left out (the stand-alone passes run their part).  hdr_blob: the chunk's header blob, which estimate and fit patch at `bits`, or null.
// With the temporal term (r.fg_denoise_span) the denoiser is two launches: the search of every frame in its neighbours on `coded` into
// d_mv (fgd_mv_entries) - in front of the filter, which on a padded chunk writes the block `coded` is - unless have_mv: d_mv holds the keys.
// estimate: off for a table the caller has put into d_fg
hipError_t launch_grain_passes(const Av1miDevParams &P, const Resolved &r, const void *tight, const void *coded, uint8_t *d_fg, uint8_t *d_fg_ar, void *out,
                               uint8_t *hdr_blob, Av1miFgBits bits, hipStream_t s, uint32_t *d_mv = nullptr, bool have_mv = false, bool estimate = true);

}  // namespace av1mi

struct av1mi_ctx {
  int device = -1;
  hipStream_t stream = nullptr;   // the four streams come from and go back to a process-wide pool (av1mi_ctx_create)
  hipStream_t stream2 = nullptr;  // CDEF + SSE run here, beside the entropy kernels on `stream`
  hipStream_t stream3 = nullptr;  // inter chunks: entropy coding of finished groups of frames, beside the frame-by-frame chain
  hipStream_t stream4 = nullptr;  // the frame-edge tiles' symbolize variant, beside the regular one on `stream` (av1mi_launch_entropy)
  hipEvent_t ev[av1mi::EV_COUNT] = {};
  std::vector<hipEvent_t> me_ev;       // per frame: its motion search has finished (second stream -> main stream)
  std::vector<hipEvent_t> grp_ev;      // per group of frames of an inter chunk: reconstructed (main stream -> third stream)
  std::string err;
  int cap_scale = 1;   // per-tile symbol-stream / bitstream-slot capacity multiplier (1, 2, 4, ... 64)
  av1mi::Workspace ws;
  Av1miDevParams P = {};
  bool sym_order = true;          // AV1MI_SYM_ORDER, read when the context is made: 0 = symbolize in natural tile order everywhere
  bool part_inter = false;        // this chunk's inter frames are partitioned from the search's node costs (partition_search = 2)
  bool quality = false;           // av1mi_ctx_set_quality: every chunk ends with the quality pass on its final frames
  bool displayed = false;         // av1mi_ctx_set_displayed_quality: every chunk with film grain ends with the synthesis and its quality pass
  const void *d_orig = nullptr;   // this chunk's frames as the caller gave them, tight, on the device: the caller's memory, d_stage or d_src
  av1mi::LastChunk last;
};

#define HIPCHK(c, call)                                                                          \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      set_err((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__);   \
      return e__ == hipErrorOutOfMemory ? AV1MI_E_OOM : AV1MI_E_HIP;                             \
    }                                                                                            \
  } while (0)

namespace av1mi {

void set_err(av1mi_ctx *c, const char *fmt, ...);
void free_workspace(av1mi_ctx *c);
int ensure_workspace(av1mi_ctx *c, const Resolved &r, uint32_t n_frames);
// whether a chunk of `r` ends with the displayed picture's quality
inline bool displayed_on(const av1mi_ctx *c, const Resolved &r) { return c->displayed && r.p.film_grain != 0; }
// the workspace's buffers bound into a chunk's parameters, each under the condition its kernels run under
void bind_workspace(Av1miDevParams &P, const Resolved &r, const Workspace &w);
// a page-locked block of the process-wide pool for a chunk's bitstream (av1mi_free puts it back); null: none to be had
void *pin_acquire(size_t bytes);
// What av1mi_file.cpp's job and caches need of the context and the two pools:
void recycle_ctx(av1mi_ctx *c);   // a context on its way into the cache of idle contexts
// the host's part of a plane's quality: the sums as av1mi_launch_quality left them at q[0 .. 1], and the plane's windows
av1mi_plane_quality plane_quality(const unsigned long long *q, const Av1miQualityGeom &G, int plane);
void expect_blocks(unsigned n);   // so many page-locked blocks may wait for a job's writer at once: park that many
void release_streams();           // destroys the stream sets destroyed contexts left in the pool
void release_buffers();           // frees the page-locked blocks av1mi_free() put back

}  // namespace av1mi

#endif
