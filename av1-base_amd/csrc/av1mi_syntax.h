// av1mi_syntax.h - the host code that needs no GPU: the parameters resolved, the headers' syntax, the default CDFs, the kernels'
// parameters as far as they follow from av1mi_params, the capacities and counts the buffers are sized by, and the scene-cut rule.
// av1mi_syntax.cpp includes no HIP header and compiles with any host C++ compiler (tests/host/syntax_host.cpp runs it under sanitizers).
#ifndef AV1MI_SYNTAX_H
#define AV1MI_SYNTAX_H
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/av1mi.h"
#include "av1mi_dev.h"

namespace av1mi {

// quantiser steps of a quantiser index, and their reciprocals ceil(2^32 / q)
struct QuantSteps { int dc_q, ac_q; uint32_t dc_recip, ac_recip; };
QuantSteps quant_steps(int qindex, int bit_depth);

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
  int tpl;                            // cq_level bits 12-14: strength of its temporal term (tpl_rule.h), 0 = off; delta_q is coded when either is set (dq_on)
  int fq;                             // cq_level bits 20-22: strength of the frame term (tpl_rule.h), 0 = off: every frame its own base_q_idx; it runs the look-ahead whatever tpl is
  uint32_t lr_fit_mask;               // enable_lr bit 8: the parameter sets the self-guided fit searches, 0 = no fit (p.enable_lr holds the type)
  int lr_wfit;                        // enable_lr bit 10: the Wiener fit (p.enable_lr holds the type)
  int lr_unit_shift;                  // enable_lr bits 12-13: luma restoration units of 64 << lr_unit_shift samples (0 .. 2)
  uint32_t lr_lambda;                 // enable_lr bits 14 and 15: the rate term's lambda (lr_rate_rule.h), 0 = the decisions go by the error alone
  int fg_estimate;                    // film_grain bit 8: the film-grain table is estimated per chunk (fg_rule.h); p.film_grain then holds the ceiling N alone
  int fg_denoise;                     // film_grain bit 10 (with bit 8): the chunk's source is denoised by the estimated table before it is coded (fg_denoise_rule.h)
  int fg_denoise_span;                // film_grain bits 14 and 15 (with bits 8 and 10): the denoiser's temporal term over so many neighbours each way, 1 or with bit 9 2; 0 = the spatial filter alone
  int fg_ar_lag;                      // film_grain bits 12-13 (with bit 8): the grain's autoregressive coefficients are fitted per chunk at this lag (fg_ar_rule.h), 0 = white grain
  int tf_frames, tf_strength;        // me_presearch bits 8-10 and 12-14: the key frames' temporal filter (tf_rule.h), 0 followers = off (p.me_presearch then holds bit 0 alone)
};

int resolve(const av1mi_params *in, Resolved *r);
// superblocks carry a quantiser index of their own: the spatial or the temporal term of the adaptive quantisation is on
inline bool dq_on(const Resolved &r) { return r.aq || r.tpl; }
// the reconstruction reads a map of quantiser indices: superblocks or frames carry an index of their own
inline bool qmap_on(const Resolved &r) { return dq_on(r) || r.fq; }
// the quantiser slots behind the parameter block and the slices of the quantiser-matrix table: 1, the 14 of the superblock terms, or the
// frame term's 28
inline int quant_slots(const Resolved &r) { return r.fq ? AV1MI_FQ_SLOTS : (dq_on(r) ? AV1MI_AQ_SLOTS : 1); }
// bytes of n frames in the caller's layout: tight at the signalled size
size_t caller_bytes(const Resolved &r, size_t n);

// sequence_header_obu, complete OBU; and the OBU_FRAME payload up to the first tile, with the bit offsets of its placeholders
std::vector<uint8_t> make_sequence_header(const Resolved &r);
std::vector<uint8_t> make_frame_header(const Resolved &r, size_t *hdr_bits, uint32_t frame_number = 0, bool inter = false, size_t *cdef_str_bit = nullptr,
                                       size_t *lf_bit = nullptr, size_t *fg_bit = nullptr, size_t *fg_ar_bit = nullptr, size_t *q_bit = nullptr);
// default CDF blob for one q context in the layout of Av1miCdfLayout
std::vector<uint16_t> make_cdf_blob(int qidx);

// per-tile capacities at multiplier `scale`, and the counts that size a chunk's buffers
int tile_slot_bytes(const Resolved &r, int scale);
int tile_stream_cap(const Resolved &r, int scale);
size_t fit_chunk_units(const Resolved &r, size_t n_frames);
size_t tf_mv_entries(const Resolved &r, size_t n_frames);
size_t fgd_mv_entries(const Resolved &r, size_t n_frames);
bool tf_runs(const Resolved &r, size_t n_frames);

// The kernels' parameters of a chunk of `n_frames` frames, as far as they follow from `r` and the capacity multiplier: every buffer
// pointer is null (av1mi_ctx.cpp binds a workspace's), and the header sizes follow with the headers (prepare_chunk).
Av1miDevParams dev_params(const Resolved &r, uint32_t n_frames, int scale);
// the block the reconstruction reads from device memory: P, then with adaptive quantisation (P.aq_map) one copy per quantiser slot
std::vector<Av1miDevParams> slot_params(const Av1miDevParams &P);
// quantiser-matrix steps of level r.qm_level (Av1miDevParams::qm_tab): one slice, or with adaptive quantisation one per quantiser slot
std::vector<Av1miQmEntry> make_qm_table(const Resolved &r);

int scene_rule_step(av1mi_scene_state *st, int has_prev, uint64_t sad, uint64_t luma_samples, int bit_depth, uint32_t min_len);

}  // namespace av1mi

#endif
