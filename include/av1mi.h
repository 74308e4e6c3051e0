/* av1mi.h - C ABI of libav1mi: the MI355X-native AV1 chunk encoder that replaces the
 * `av1an` -> SVT-AV1 subprocess behind the av1-base daemon's encode boundary.
 *
 * Every entry point names the reference interface (file:line under /root/reference) it
 * replaces.  Plain C types only: no C++/torch types cross this boundary; nothing throws.
 *
 * Error convention (maps 1:1 onto the reference's `EncodeError`,
 * crates/daemon/src/encode/av1an.rs:17-30):
 *     0            -> Ok(())
 *     > 0          -> EncodeError::Av1anFailed(code)      (encoder / GPU failure; see AV1MI_E_*)
 *     < 0 (-errno) -> EncodeError::Io(io::Error::from_raw_os_error(errno))
 * `Av1anTerminated` (killed by signal) has no in-process equivalent.
 */
#ifndef AV1MI_H
#define AV1MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AV1MI_ABI_VERSION 8

/* positive failure codes (-> Av1anFailed(code)) */
enum {
  AV1MI_OK = 0,
  AV1MI_E_INVALID_ARG = 1,   /* bad dimensions / parameters */
  AV1MI_E_NO_DEVICE = 2,     /* no MI355X visible, or HIP runtime failure at init */
  AV1MI_E_HIP = 3,           /* a HIP call or kernel failed; see av1mi_last_error() */
  AV1MI_E_OOM = 4,           /* host or device allocation failed */
  AV1MI_E_OVERFLOW = 5,      /* a tile outgrew its bitstream slot */
  AV1MI_E_FORMAT = 6,        /* input file is not a supported Y4M (420, 8/10 bit) */
  AV1MI_E_UNSUPPORTED = 7    /* valid request this build cannot serve yet (e.g. frames wider than 64 superblocks) */
};

typedef struct av1mi_ctx av1mi_ctx;

/* av1mi_params.cq_level carries four values: the CQ level, the strength of the adaptive quantisation's spatial term, the strength
 * of its temporal term and the strength of the frame term (every frame its own base_q_idx) */
#define AV1MI_CQ_AQ(cq, strength) (((uint32_t)(cq) & 0xFFu) | (((uint32_t)(strength) & 7u) << 8))
#define AV1MI_CQ_AQ_TPL(cq, aq, tpl) (AV1MI_CQ_AQ(cq, aq) | (((uint32_t)(tpl) & 7u) << 12))
#define AV1MI_CQ_AQ_TPL_FQ(cq, aq, tpl, fq) (AV1MI_CQ_AQ_TPL(cq, aq, tpl) | (((uint32_t)(fq) & 7u) << 20))
#define AV1MI_CQ_LEVEL(v) ((uint32_t)(v) & 0xFFu)
#define AV1MI_AQ_STRENGTH(v) (((uint32_t)(v) >> 8) & 7u)
#define AV1MI_TPL_STRENGTH(v) (((uint32_t)(v) >> 12) & 7u)
#define AV1MI_FQ_STRENGTH(v) (((uint32_t)(v) >> 20) & 7u)
/* av1mi_params.enable_lr with the self-guided fit: lr = 2 or 4, sets = a mask over the 16 parameter sets searched (0 = all) */
#define AV1MI_LR_FIT(lr, sets) ((uint32_t)(lr) | 0x100u | ((uint32_t)(sets) << 16))
/* av1mi_params.enable_lr bit 10: the Wiener fit, or-ed into a value with a low byte of 1 .. 4 (with or without AV1MI_LR_FIT) */
#define AV1MI_LR_WIENER_FIT 0x400u
/* av1mi_params.enable_lr bits 12-13: lr_unit_shift, or-ed into a value with a low byte of 1 .. 4 (with or without either fit) -
 * restoration units of 128x128 / 256x256 luma samples instead of 64x64 */
#define AV1MI_LR_UNIT_128 0x1000u
#define AV1MI_LR_UNIT_256 0x2000u
#define AV1MI_LR_UNIT_SHIFT(v) (((uint32_t)(v) >> 12) & 3u)
/* av1mi_params.enable_lr bits 14 and 15, both: the unit decisions weigh a rate term, or-ed into a value with a low byte of 1 .. 4 (with
 * or without either fit and a unit size); s = 0 .. 3 scales lambda by 1, 1/2, 1/4, 2: bit 0 of s is bit 9 of the field, bit 1 is bit 11 */
#define AV1MI_LR_RD(s) (0xC000u | (((uint32_t)(s) & 1u) << 9) | (((uint32_t)(s) & 2u) << 10))
#define AV1MI_LR_RD_ON(v) (((uint32_t)(v) & 0xC000u) == 0xC000u)
#define AV1MI_LR_RD_SCALE(v) ((((uint32_t)(v) >> 9) & 1u) | (((uint32_t)(v) >> 10) & 2u))
/* av1mi_params.me_presearch carries three values: bit 0 the pre-search's switch, bits 8-10 the frames (0 = off, 1 .. 7) and bits 12-14
 * the strength (0 .. 7) of the key frames' temporal filter */
#define AV1MI_ME_TF(presearch, frames, strength) (((uint32_t)(presearch) & 1u) | (((uint32_t)(frames) & 7u) << 8) | (((uint32_t)(strength) & 7u) << 12))
#define AV1MI_ME_PRESEARCH(v) ((uint32_t)(v) & 1u)
#define AV1MI_TF_FRAMES(v) (((uint32_t)(v) >> 8) & 7u)
#define AV1MI_TF_STRENGTH(v) (((uint32_t)(v) >> 12) & 7u)
/* av1mi_params.film_grain with the table estimated from the chunk's source: N = 1 .. 50 stays the ceiling of its values */
#define AV1MI_FILM_GRAIN_ESTIMATE(n) ((uint32_t)(n) | 0x100u)
#define AV1MI_FILM_GRAIN_ESTIMATED(v) ((((uint32_t)(v)) >> 8) & 1u)
#define AV1MI_FILM_GRAIN_LEVEL(v) ((uint32_t)(v) & 0xFFu)
/* ... and with the source denoised by that table before it is coded (bit 10, only together with bit 8) */
#define AV1MI_FILM_GRAIN_DENOISE(n) ((uint32_t)(n) | 0x100u | 0x400u)
#define AV1MI_FILM_GRAIN_DENOISED(v) ((((uint32_t)(v)) >> 10) & 1u)
/* ... and with the grain's autoregressive coefficients fitted at lag 1 .. 3 (bits 12-13, only together with bit 8): or-ed into either of
 * the two values above */
#define AV1MI_FILM_GRAIN_AR(lag) (((uint32_t)(lag) & 3u) << 12)
#define AV1MI_FILM_GRAIN_AR_LAG(v) ((((uint32_t)(v)) >> 12) & 3u)
/* ... and the denoiser with its motion-compensated temporal term over span = 1 or 2 neighbour frames each way (bits 14 and 15, both, only
 * together with bits 8 and 10; bit 9, only together with them, selects span 2); AV1MI_FILM_GRAIN_AR(L) may be or-ed in.  _SPAN: 0, 1 or 2 */
#define AV1MI_FILM_GRAIN_DENOISE_TEMPORAL(n, span) ((uint32_t)(n) | 0x100u | 0x400u | 0xC000u | ((span) == 2 ? 0x200u : 0u))
#define AV1MI_FILM_GRAIN_DENOISE_SPAN(v) ((((uint32_t)(v)) & 0xC000u) == 0xC000u ? ((((uint32_t)(v)) & 0x200u) ? 2u : 1u) : 0u)

/* Operating point.  Replaces the reference's single constant
 *   SVT_PARAMS = "--crf 8 --preset 3 --film-grain 20 ... --keyint 240 --lookahead 40"
 * (crates/daemon/src/encode/av1an.rs:14) and `--pix-format yuv420p10le` (av1an.rs:90).  What `--lookahead` buys there has three
 * switches here, all off by default and all over the whole chunk rather than 40 frames: the key frames' temporal filter
 * (me_presearch, AV1MI_ME_TF), the temporal-dependency term of the adaptive quantisation (cq_level, AV1MI_CQ_AQ_TPL) and every
 * frame's own base_q_idx from the same analysis (cq_level, AV1MI_CQ_AQ_TPL_FQ).  The deblocking level and the quantiser-matrix level do
 * not follow the frame's index, and there is no B pyramid. */
typedef struct {
  uint32_t width, height;   /* luma size, even, >= 8, yuv 4:2:0.  Sizes that are not multiples of 8 are coded at the next
                               multiple of 8 (source edge-extended on the device) and signalled exactly, as any AV1 encoder does */
  uint32_t bit_depth;       /* 8 or 10 (samples: uint8_t / little-endian uint16_t) */
  uint32_t cq_level;        /* bits 0-7: "--crf N": 1..63, mapped to base_q_idx like aom (30 -> 120).  0 (base_q_idx 0: lossless
                               coding, which this encoder does not do) is refused with AV1MI_E_INVALID_ARG.
                               bits 8-10: aq_strength 0..4, activity-adaptive quantisation (AV1MI_CQ_AQ packs the field; DESIGN.md §3
                               item 1c): 0 (default) = one quantiser index per frame; s = 1..4: every 64x64 superblock gets
                               base_q_idx + 4 d, d in -6..6 from s times the difference between the log2 variance of its source luma
                               (mean over its 8x8 units) and the frame's mean, s = 2 being one step per doubling - flat superblocks a
                               finer quantiser, busy ones a coarser (delta_q_present = 1, delta_q_res = 2; deblocking level, partition
                               threshold and quantiser-matrix level stay with base_q_idx).
                               bits 12-14: tpl_strength 0..4, the temporal term of the same map (AV1MI_CQ_AQ_TPL packs the field;
                               DESIGN.md §3 item 1d): 0 (default) = off; s = 1..4: a look-ahead over the whole chunk follows the
                               motion of 16x16 source blocks (whole samples, +-me_range, frame against the frame before) backwards
                               from the chunk's last frame and measures, per superblock, beta = the log2 of how much of the later
                               frames it is going to predict; s (beta - the chunk's mean beta) is subtracted from the spatial term
                               before d is formed - superblocks the rest of the chunk depends on a finer quantiser, superblocks
                               nothing depends on a coarser.  Either strength alone turns delta_q_present on; with keyint = 1
                               nothing is predicted and the term is 0.
                               bits 20-22: fq_strength 0..4, the frame term (AV1MI_CQ_AQ_TPL_FQ packs the field):
                               0 (default) = every frame of the chunk at the index the CQ level maps to; s = 1..4: the same look-ahead
                               (it runs whatever tpl_strength is) gives every frame betaF = the log2 of (its own cost + what the later
                               frames take from it) / its own cost, and the frame is coded at base_q_idx + 4 k, k in -10..+4 from
                               s (betaF - the chunk's mean betaF), s = 1 being one step per doubling - the first frame of a long
                               interval a finer quantiser, the last frame in front of a key frame, which nothing depends on, a
                               coarser.  The frame's header carries its index; the coefficient CDFs' q context, CurrentQIndex at the
                               tile starts and the quantiser follow it.  With a superblock strength as well the temporal term is taken
                               against the frame's own mean beta and d is clamped against the frame's index.  What stays with the
                               chunk's index, each an encoder's choice and legal in the stream: the deblocking level and the level
                               search's centre, both partition thresholds, the quantiser-matrix level, the restoration's lambda, the
                               inter-partition penalty and the range coder's stage choice.  delta_q_present stays "aq_strength or
                               tpl_strength".  Strengths 5..7 of any of the three, bits 11, 15-19 and 23-31 are refused with
                               AV1MI_E_INVALID_ARG */
  uint32_t keyint;          /* "--keyint": 1 = every frame a key frame; N > 1 = a key frame every N frames of a chunk, the
                               frames between are INTER frames predicted from the previous reconstruction (one
                               reference, integer-pel full search; chunks always start with a key frame) */
  uint32_t block_log2;      /* leaf block size log2: 3 (8x8) .. 6 (64x64: 64-point luma transforms, of which AV1 codes the 32x32
                               low-frequency corner); 0 = default (5) */
  uint32_t cdf_update;      /* 1 = adaptive CDFs (default), 0 = static CDFs (disable_cdf_update) */
  uint32_t enable_cdef;     /* 1 = CDEF on (default) */
  uint32_t cdef_y_pri, cdef_y_sec, cdef_uv_pri, cdef_uv_sec, cdef_damping; /* 0s = defaults */
  uint32_t intra_mode_mask; /* bit m = luma intra mode m is a candidate (AV1 mode numbering); 0 = default {DC, V, H} */
  uint32_t film_grain;      /* "--film-grain N" (av1an.rs:14): 0 = off; N = 1..50 writes a film-grain table into every
                               frame header (2-point scaling functions, value 2N luma / N chroma, AR lag 0);
                               synthesis is decoder-side.
                               bit 8 with a low byte N = 1..50 (AV1MI_FILM_GRAIN_ESTIMATE(N)): the table is
                               estimated per chunk from the chunk's own source, on the GPU, as SVT-AV1's "--film-grain N" measures
                               its source - per plane eight points at x = 16 + 32 k whose values are, per luma intensity bin, the
                               lower quartile over the chunk's whole 16x16 blocks (with their 8x8 chroma blocks) of a noise estimate
                               that is blind to planes and ramps, scaled to the table's units (fg_rule.h).  N stays the ceiling: no
                               luma value exceeds 2N and no chroma value N, the fixed table's values, so the estimate never adds
                               more grain than film_grain = N - on a clean source it adds less, down to none.  The same table goes
                               into every frame of the chunk; the frame header is 288 bits longer than the fixed mode's, whatever
                               the content; tile data and reconstruction are those of the fixed mode.  av1mi_write_headers returns
                               the header with the ceiling's values, av1mi_film_grain_result the chunk's table.
                               bit 10 together with bit 8 (AV1MI_FILM_GRAIN_DENOISE(N)): the second half
                               of "--film-grain N" - the chunk is coded from a source with the measured grain taken out, and the
                               decoder puts it back by synthesis.  After the estimate, which still reads the frames as the caller
                               gave them, every sample of the three planes is replaced by a weighted mean over its 5x5 window
                               whose weights fall linearly with the difference from the sample and reach 0 at T = 4 sigma of the
                               grain the table signals at the sample's luma (fg_denoise_rule.h) - a zero table changes nothing,
                               no sample moves by T or more.  The key frames' temporal filter, the partition, the adaptive
                               quantisation and the encoder proper see the denoised chunk; av1mi_report.sse and psnr are against
                               it (the coded source, as with the temporal filter).  Headers and av1mi_film_grain_result are the
                               estimate mode's; the caller's frames are never written.
                               bits 12-13 = L = 1..3 together with bit 8, with or without bit 10 (| AV1MI_FILM_GRAIN_AR(L); DESIGN.md
                               section 3 item 7d): the third piece - the grain the decoder synthesises gets the source grain's
                               size instead of being white.  After the estimate, and on the same frames, the blocks the table calls
                               flat (value at most their bin's quartile, detrended energy at most 16 sigma^2 of it) are detrended
                               by their least-squares plane, the products of their residuals at the offsets a lag-L filter sees
                               are summed over the chunk per plane, and the 2 L (L + 1) coefficients per plane are fitted to the
                               resulting correlations and quantised to Q7, ar_coeff_shift_minus_6 = 1 (fg_ar_rule.h, all integers).
                               The points of a plane are scaled by the square root of the innovation's share of the variance, so
                               the synthesised grain keeps the sigma the estimate measured; a plane without 16 flat blocks or
                               with an ill-conditioned or amplifying fit keeps zero coefficients and its points.  The chroma
                               planes' luma tap stays 0.  The frame header is 48 L (L + 1) bits longer than the estimate mode's,
                               whatever the content; tile data and reconstruction are those of the same mode with L = 0; the
                               denoiser keeps the unscaled table.  av1mi_write_headers returns ceiling values and zero coefficients,
                               av1mi_film_grain_result the scaled table, av1mi_film_grain_ar_result the rest.
                               bits 14 and 15, both, together with bits 8 and 10 (AV1MI_FILM_GRAIN_DENOISE_TEMPORAL(N, span);
                               DESIGN.md section 3 item 7e): the denoiser's temporal term.  Grain is independent from frame to
                               frame, the picture is not: per 16x16 luma block every frame f is searched (whole samples, +-me_range
                               around zero, the undenoised frames at the coded size) in each neighbour g = f - S .. f + S of the
                               chunk, S = 1, or 2 with bit 9, across key frames; on top of its 5x5 window every sample takes the
                               3x3 window of the caller's undenoised frame g around the displaced position (chroma: the vector
                               halved, whole samples), with the same weights by the same T - the centre counting four times - so
                               a wrong match weighs nothing.  A zero table still changes nothing, no sample moves by T or more,
                               and a one-frame chunk is the spatial filter's.  Headers and av1mi_film_grain_result stay the
                               estimate mode's.
                               Bit 8 with a low byte of 0 or above 50, bit 10 or bits 12-13 without bit 8, bit 14 or bit 15 alone or
                               without bit 10, bit 9 without bits 14 and 15, bit 11, any bit above 15, and 51..255 are refused with
                               AV1MI_E_INVALID_ARG.  A context may switch the mode, the span and the lag from chunk to chunk */
  uint32_t first_frame;     /* number of the chunk's first frame inside the clip (seeds grain_seed per frame) */
  uint32_t me_range;        /* inter frames: motion search range in luma samples, 8 or 16 (0 = 8) */
  uint32_t enable_lr;       /* 1 = loop restoration on luma (Wiener, 64x64 units, each unit off or one of 3 filters by SSE);
                               2 = RESTORE_SWITCHABLE: each unit off, one of the 3 Wiener filters or one of 3 self-guided
                               filters (parameter set 9, three weightings);
                               3 / 4 = 1 / 2 on all three planes: U and V in 32x32 units (the picture area of a luma
                               unit), each unit decided on its own; chroma Wiener filters (0, 0, -4), (0, 0, 16), (0, 6, 20).
                               A library without chroma restoration refuses 3 and 4 with AV1MI_E_INVALID_ARG, as every
                               library refuses values above 4 in the low byte;
                               bit 8 with a low byte of 2 or 4 (AV1MI_LR_FIT packs the field): the
                               self-guided filter is fitted per unit - beside the seven candidates above a unit may take any of
                               the 16 parameter sets (bits 16-31: a mask over the sets searched, 0 = all) with the two weights
                               that least squares gives for the unit, the smallest exact SSE winning as before.  Headers are
                               those of 2 / 4.  Bit 8 with any other low byte, and bits 9, 11, 14 and 15 (but see AV1MI_LR_RD below), are refused with
                               AV1MI_E_INVALID_ARG.  av1mi_lr_fit_result reports the units' choices;
                               bit 10 (AV1MI_LR_WIENER_FIT) with a low byte of 1 .. 4, alone or with
                               bit 8: after the decision above a unit's Wiener filter is fitted by least squares - three vertical
                               and three horizontal taps (chroma: two and two) - and replaces the unit's winner where its exact
                               SSE is strictly smaller.  Headers are those of the low byte.  Bit 10 with any other low byte is
                               refused with AV1MI_E_INVALID_ARG.  av1mi_lr_wiener_fit_result reports the units' final choices;
                               bits 12-13 (AV1MI_LR_UNIT_128, AV1MI_LR_UNIT_256) with a low byte of
                               1 .. 4, alone or with bit 8, bit 10 or both: lr_unit_shift 1 / 2 - luma units of 128x128 / 256x256
                               samples, chroma units of half that (always the picture area of a luma unit), max(1, (size + U / 2) / U)
                               units each way; every decision, fit and result above is then taken per unit of that size, and a unit
                               signals a quarter / a sixteenth of the side information.  The frame header grows by one bit.  Both
                               bits set, and either with a low byte of 0, are refused with AV1MI_E_INVALID_ARG.  A context may
                               change the unit size from chunk to chunk;
                               bits 14 and 15, both (AV1MI_LR_RD(s)) with a low byte of 1 .. 4 and any of
                               the bits above: every unit decision - fixed candidates, self-guided fit, Wiener override, all planes,
                               all unit sizes - minimises J = 16 D + lambda B16 instead of the squared error D.  B16 is the unit's
                               side information in sixteenths of a bit: its coefficients' length against the tile-start reference
                               plus its type symbol under the default CDFs; lambda = (13 q^2) >> 9 from the dc step q of base_q_idx,
                               scaled by s = 0 .. 3 (bits 9 and 11 of the field): x1, x1/2, x1/4, x2.  Filters, fits, candidate order,
                               syntax and headers are unchanged.  Bits 9, 11, 14 or 15 without both of 14 and 15 stay refused with
                               AV1MI_E_INVALID_ARG, as do both with a low byte of 0 or above 4.  A context may switch the mode from
                               chunk to chunk.  av1mi_lr_rd_result reports the units' final choices and bits;
                               default 0: the decision needs the CDEF output, which serialises CDEF before entropy coding */
  uint32_t tile_sb;         /* tile size in 64x64 superblocks, both ways: 0 = automatic (1; 2 when the frame has more than 64
                               superblock rows or columns, e.g. 8K - AV1 allows at most 64 x 64 tiles), or force 1 / 2 */
  uint32_t deblock;         /* 1 = deblocking filter on (default 0: `loop_filter_level` = 0); the level follows the quantiser:
                               g = (ac_q * 20723 + 1015158) >> 18 at 8-bit scale, 4 less on key frames, all four filters alike.
                               2 = the level is searched on the GPU per frame and per plane: 16
                               candidates g + {-12, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 12, 16} clamped to 1..63 (luma)
                               / 0..63 (U, V); each plane takes the first candidate with the least squared error of the deblocked
                               plane against the source, luma one level for both edge directions.  Sharpness stays 0, no
                               loop-filter deltas.  av1mi_lf_search_result reports the levels.  Values above 2 are refused
                               with AV1MI_E_INVALID_ARG (before the search existed every nonzero value meant 1) */
  uint32_t enable_qm;       /* "--enable-qm 1" (av1an.rs:14): quantiser matrices (using_qmatrix).  The level of all three planes
                               follows the quantiser as in SVT-AV1/libaom: qm_min + base_q_idx * (qm_max + 1 - qm_min) / 256
                               (0 = steepest matrix ... 14; 15 = flat).  Default 0 */
  uint32_t qm_min, qm_max;  /* "--qm-min" / "--qm-max": 0..15, qm_min <= qm_max; av1mi_default_params sets 8 / 15 (the encoder's
                               defaults); the reference's production string uses 1 / 15 */
  uint32_t subpel;          /* inter frames: 1 = quarter-sample motion vectors (the full search's winner refined over its half- and then
                               quarter-sample neighbours) predicted with the 8-tap EIGHTTAP filter; 0 (default) = whole-sample
                               vectors, frame filter BILINEAR */
  uint32_t color_range;     /* color_config.color_range of the sequence header: 0 (default) = studio / limited range - what Y4M input and the
                               reference's pipeline (ffmpeg -> SVT-AV1, `--pix-format yuv420p10le`, av1an.rs:90) carry; 1 = full range.
                               av1mi_encode_file takes it from the Y4M header's XCOLORRANGE tag when there is one */
  uint32_t intra_angle_delta; /* 1: a directional winner of the luma mode decision (V, H, D45 .. D67) is refined over the angle deltas
                               -3 .. +3 (3 degrees each) by closed-loop SAD, chroma follows luma; 0 (default): delta 0 */
  uint32_t intra_edge_filter; /* sequence header enable_intra_edge_filter (SVT-AV1 and libaom run with it on): 1 = directional intra
                               predictions read the filtered / upsampled edges of AV1 spec 7.11.2.7 - 7.11.2.12; 0 (default) */
  uint32_t cfl;             /* 1: chroma-from-luma prediction (UV_CFL_PRED, AV1 spec 7.11.5) is a candidate for the chroma planes of key-frame
                               blocks up to 32x32 (alpha per plane by least squares over the reconstructed luma); 0 (default) */
  uint32_t tx_search;       /* 1: transform type search - intra luma blocks up to 16x16 whose residual is sparse (at most one sample in
                               eight nonzero) are coded with the identity transform (IDTX); 0 (default): the mode's default type */
  uint32_t color_primaries, transfer_characteristics, matrix_coefficients;
                            /* color_config's colour description (AV1 spec 5.5.2; CICP / ISO 23091-2 code points), written into the sequence
                               header and, for Matroska output, the track's Colour element: what the reference's ffmpeg -> SVT-AV1 pipeline
                               passes through (`--pix-format yuv420p10le`, av1an.rs:90).  All 0 (default) = no description
                               (color_description_present_flag 0); BASELINE config 5 "8K 10-bit HDR" = 9 / 16 / 9 (BT.2020 primaries, SMPTE
                               2084 PQ, BT.2020 non-constant luminance).  Values 0..255 each; the triple 1 / 13 / 0 (sRGB + identity) implies
                               4:4:4 and is refused */
  uint32_t partition_search; /* 1: content-driven partition - a node of the partition tree larger than `min_block_log2` and not larger than `block_log2`
                               splits when its four quadrants differ in activity (largest quadrant variance of the source luma > 4 x the
                               smallest + (ac_q / 16)^2), so quiet areas keep large blocks and edges / small objects get small ones; decided
                               for all frames of a chunk by one GPU pass over the source.  2: key frames as with 1; an inter frame's
                               nodes are decided bottom up from the motion search's block costs instead - the search keeps the best
                               candidate of every node of the tree, and a node splits iff its children's costs plus a penalty of
                               (n^2 (ac_q / 16)) >> 3 undercut its own (av1mi_inter_partition_result reports
                               the masks).  3 and above are refused.  0 (default): every block is `block_log2` */
  uint32_t min_block_log2;  /* smallest leaf under partition_search: 3 (8x8, default when 0) .. block_log2 */
  uint32_t me_presearch;    /* inter frames: 1 = hierarchical motion search - a quarter-resolution search of +-64 luma samples per 32x32 cell finds the
                               centre the full-resolution search of +-me_range then runs around (row a13's "1/4-res ... full"); 0 (default): the
                               full-resolution search runs around the zero vector.
                               bits 8-10: tf_frames N = 1 .. 7, bits 12-14: tf_strength s = 0 .. 7 (AV1MI_ME_TF packs the field) - the key
                               frames' temporal filter: every key frame f (f % keyint == 0) of a chunk is
                               replaced, as the source of the whole encode, by its motion-compensated filter over the frames f + 1 ..
                               f + min(N, keyint - 1, frames left in the chunk); the caller's frames are not written, followers are not
                               changed, and the bitstream is the one the chunk with av1mi_temporal_filter's output gives with the filter
                               off.  N = 0 (default): off.  Any other bit, or s without N, is refused */
  uint32_t cdef_search;     /* CDEF strengths chosen per frame and per 64x64 superblock by an exhaustive search on the device:
                               0 (default) = off, the fixed strengths above for every frame; k = 1..4 = on, cdef_bits = k - 1, i.e. 1, 2, 4 or 8
                               strength pairs per frame, each superblock picking one by the squared error of the filtered output against the
                               source.  With the search on cdef_y_pri, cdef_y_sec, cdef_uv_pri and cdef_uv_sec are ignored; cdef_damping still
                               applies (0: the default, 5).  Values above 4, or any value but 0 with enable_cdef = 0, are refused */
} av1mi_params;

typedef struct {
  uint8_t *data;            /* owned by the library (a page-locked block of its pool, or malloc); release with av1mi_free() ONLY */
  size_t size;
} av1mi_buf;

/* per-chunk report: fills the reference's hollow JobMetrics fields `fps, frames_encoded, psnr`
 * (crates/daemon/src/metrics.rs:12-30; zeros today at job_executor.rs:117-137) */
typedef struct {
  uint32_t frames;
  uint64_t bytes;
  double sse[3];            /* sum of squared error of the reconstruction, per plane: against the coded source - with the temporal
                               filter on, the filtered key frames (av1mi_temporal_filter returns them), with the film-grain denoiser
                               on, the denoised frames (av1mi_film_grain_denoise returns them), not the caller's */
  double psnr[3];           /* ... and the PSNR from it, likewise */
  /* device time per stage, milliseconds (HIP events on the encoder's stream) */
  float ms_h2d, ms_recon, ms_cdef, ms_entropy, ms_pack, ms_d2h, ms_total;
  float ms_symbolize;       /* part of ms_entropy spent in the symbolize kernel */
  uint64_t n_symbols;       /* arithmetic-coded symbols */
  uint32_t max_tile_symbols; /* longest tile: the serial chain that bounds the range-coding kernel */
  uint32_t cap_scale;       /* per-tile capacity multiplier the chunk finally ran with (1 unless a tile overflowed
                               and the chunk was re-run) */
  uint32_t chunks;          /* av1mi_encode_file: chunks the clip was split into (1 for av1mi_encode_chunk) */
  uint32_t gpus_used;       /* bit d = GPU d encoded at least one chunk of the job (av1mi_encode_chunk: the context's device) - what
                               `gpu_mask` and av1mi_plan_workers resolved to on this host */
} av1mi_report;

void av1mi_default_params(av1mi_params *p, uint32_t width, uint32_t height, uint32_t bit_depth);

/* One context = one GPU + one HIP stream = one chunk in flight.  `workers` of the reference's
 * ConcurrencyPlan (crates/daemon/src/concurrency.rs:9-18 -> `--workers`, av1an.rs:100-101)
 * becomes "number of contexts".  Thread-safe across contexts; one thread per context. */
int av1mi_ctx_create(int device_id, av1mi_ctx **out);
void av1mi_ctx_destroy(av1mi_ctx *ctx);
const char *av1mi_last_error(const av1mi_ctx *ctx);

/* Encode one scene-chunk: `n_frames` planar I420 frames, frame k at
 * `frames + k * frame_bytes` with frame_bytes = w*h*3/2*bytes_per_sample (Y then U then V) -
 * the unit av1an hands to one SVT-AV1 worker.  `frames_on_device` != 0: `frames` is a device
 * pointer (HBM-resident input).  Output: a Section-5 OBU stream (temporal delimiter + sequence
 * header + OBU_FRAME per frame); `frame_sizes` (optional, n_frames entries) receives each
 * temporal unit's size.  `recon` (optional, same layout/pointer kind as `frames`) receives the
 * decoder-identical reconstruction.  Blocking; returns the error codes above. */
int av1mi_encode_chunk(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames,
                       int frames_on_device, av1mi_buf *out, uint32_t *frame_sizes, void *recon,
                       av1mi_report *report);

void av1mi_free(void *p);

/* ---- scene-cut detection (the chunker) ----------------------------------------------------
 * Replaces the scene detection av1an performs before it hands chunks to its `--workers N` encoders
 * (`--workers`, `--temp`: crates/daemon/src/encode/av1an.rs:100-104).
 * Device: SAD of every frame's luma against its predecessor (one streaming kernel).  Host: frame t
 * starts a new scene iff  2*d(t) >= 5*mean(d over the last <= 8 in-scene frames)  and  d(t) >= 8
 * (d = mean absolute luma difference at 8-bit scale, Q8 integers; with no history yet: d(t) >= 24)
 * and the current scene already holds `min_scene_len` frames.  A frame without predecessor
 * (`prev_frame` NULL and t = 0) always starts a scene.  `state` (zero-initialised by the caller) carries
 * the history across calls so a clip can be streamed window by window; `prev_frame` is the last frame of
 * the previous window (same residency as `frames`).  Outputs (each n_frames entries, optional):
 * `sad` = luma SAD against the predecessor (0 for a frame without one), `is_cut` = 1 where a scene starts. */
typedef struct {
  uint32_t frames_since_cut;
  uint32_t hist_n;
  uint32_t hist_q8[8];
} av1mi_scene_state;

int av1mi_scene_cuts(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames,
                     int frames_on_device, const void *prev_frame, av1mi_scene_state *state,
                     uint32_t min_scene_len, uint64_t *sad, uint8_t *is_cut);

/* ---- adaptive quantisation: the decision on its own (what an analysis tool wants) ------------
 * The quantiser index every 64x64 superblock of every frame is coded with: qindex[(f * sb_rows + r) * sb_cols + c],
 * sb_cols = (ceil8(width) + 63) / 64, likewise rows; all base_q_idx when both strengths are 0; with a tpl_strength the map of both
 * terms, the frames taken as one chunk (keyint and me_range as the parameters say).  Same frame arguments as
 * av1mi_scene_cuts (tight planar frames, host or 16-byte aligned device memory). */
int av1mi_aq_qindex(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames,
                    int frames_on_device, uint8_t *qindex);

/* ---- the temporal-dependency analysis on its own ----------------------------------------------
 * What av1mi_encode_chunk runs on a chunk's source when av1mi_params.cq_level carries a tpl_strength (AV1MI_CQ_AQ_TPL): the same
 * launches on the same frames, taken as one chunk.  Every output is optional, host memory.  Per frame f and 16x16 block b of the
 * coded size (nb = ceil(ceil8(width) / 16) * ceil(ceil8(height) / 16) blocks in raster order), at [f * nb + b]: intra = I, the block's
 * sum of absolute differences from its mean (at least 1); inter = C, min(I, the SAD of the best whole-sample vector within +-me_range
 * against frame f - 1), I on key frames; key = that vector's (cost << 11) | index as av1mi_temporal_filter reports its own,
 * 0xFFFFFFFF on key frames; flow = A, what the frames after f inside its key-frame interval hand back to the block.  beta: per frame
 * and superblock, layout of av1mi_aq_qindex: 16 log2 ((sum I + A) / sum I) over the superblock's blocks; *mean_beta: its rounded mean
 * over the chunk.  AV1MI_E_INVALID_ARG when the strength is 0.  Like av1mi_aq_qindex it looks at the frames it is given. */
int av1mi_tpl_analysis(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                       uint32_t *intra, uint32_t *inter, uint32_t *key, uint64_t *flow, uint16_t *beta, uint32_t *mean_beta);

/* ---- the frame term on its own ------------------------------------------------------------------
 * What av1mi_encode_chunk runs on a chunk's source when av1mi_params.cq_level carries an fq_strength (AV1MI_CQ_AQ_TPL_FQ): the same
 * launches on the frames it is given, taken as one chunk.  Every output is optional, host memory, one entry per frame: intra_sum =
 * OF, the sum of I over the frame's 16x16 blocks; dep_sum = PF, the sum of I + A; beta = betaF = 16 log2 (PF / OF) as the analysis
 * forms it; *mean_beta = MF, its rounded mean over the frames; frame_q = the frame's base_q_idx.  AV1MI_E_INVALID_ARG when the
 * strength is 0; arguments are checked before a device is touched.  With an fq_strength av1mi_aq_qindex returns the combined map,
 * the frames' steps included, and av1mi_write_headers the header with the chunk's index as the placeholder the device overwrites. */
int av1mi_tpl_frame_q(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                      uint64_t *intra_sum, uint64_t *dep_sum, uint16_t *beta, uint32_t *mean_beta, uint8_t *frame_q);
/* The same of the chunk the context encoded last: frame_q[n_frames] and beta[n_frames] (each optional) - all base_q_idx and zeros for
 * a chunk without the term.  AV1MI_E_INVALID_ARG without a successfully encoded chunk or with another frame count. */
int av1mi_frame_q_result(const av1mi_ctx *ctx, uint32_t n_frames, uint8_t *frame_q, uint16_t *beta);

/* ---- the key frames' temporal filter on its own --------------------------------------------
 * What av1mi_encode_chunk codes instead of the key frames when av1mi_params.me_presearch carries the filter (AV1MI_ME_TF): the
 * same launches on the same frames.  `out` (optional; layout and residency of `frames`, at the signalled size): the chunk with
 * its key frames filtered and every other frame copied.  `mv` (optional, host memory): the filter's motion search,
 * mv[((f / keyint) * N + (t - 1)) * nb + b] = the winner of block b of key frame f against frame f + t as (cost << 11) | index,
 * cost = SAD + 16 (|dx| + |dy|), index = (dy + R) (2 R + 1) + dx + R, R = me_range; nb = the 16x16 blocks of the coded size
 * (width and height rounded up to multiples of 8), b in raster order; 0xFFFFFFFF for a follower that does not exist.  With the
 * filter off `out` is a copy and `mv` is not written.
 * av1mi_aq_qindex and av1mi_scene_cuts look at the frames they are given, whatever the field says: a caller who wants what the
 * encoder sees with the filter on passes them this call's output. */
int av1mi_temporal_filter(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames,
                          int frames_on_device, void *out, uint32_t *mv);

/* ---- the film-grain estimate on its own ---------------------------------------------------------
 * What av1mi_encode_chunk runs on a chunk's source when av1mi_params.film_grain carries bit 8 (AV1MI_FILM_GRAIN_ESTIMATE): the same
 * launches on the same frames, taken as one chunk.  Every output is optional, host memory.  table[plane * 8 + k]: the value of point k
 * (x = 16 + 32 k) of plane 0 .. 2 (Y, U, V), what the chunk's frame headers carry.  counts[plane * 8 + k]: the blocks of luma bin k
 * (equal for the three planes); a bin below 16 blocks took its value from the nearest bin that has them.  blocks: per frame f and whole
 * 16x16 block b of the signalled size (nb = (width / 16) * (height / 16) blocks in raster order), at [(f * nb + b) * 4 + 0..3]:
 * { bin, v_y, v_u, v_v }, the block's luma bin and its three noise values before the quartile and the ceiling.  AV1MI_E_INVALID_ARG
 * without bit 8; the arguments are checked before a device is touched.  Like av1mi_aq_qindex it looks at the frames it is given. */
int av1mi_film_grain_estimate(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                              uint8_t *table, uint32_t *counts, uint8_t *blocks);
/* The table the frame headers of the context's last successfully encoded chunk carry, layout as above; zeros for a chunk without the
 * estimate.  The values arrive with the chunk's other small results: the call only copies them.  AV1MI_E_INVALID_ARG without such a chunk. */
int av1mi_film_grain_result(const av1mi_ctx *ctx, uint8_t *table);

/* ---- the film-grain denoiser on its own ------------------------------------------------------------
 * What av1mi_encode_chunk runs on a chunk's source when av1mi_params.film_grain carries bits 8 and 10 (AV1MI_FILM_GRAIN_DENOISE): the
 * same launches on the same frames, taken as one chunk.  out: the denoised chunk at the signalled size, in the layout and residency of
 * `frames` (device pointers 16-byte aligned, a block other than `frames`).  table (optional, host): the 24 values [plane * 8 + k] the
 * filter ran with.  use_table (optional, host): 24 values the filter takes as they are instead of the chunk's estimate - no ceiling is
 * applied and the estimate is skipped.  AV1MI_E_INVALID_ARG without bits 8 and 10; the arguments are checked before a device is touched.
 * Like av1mi_film_grain_estimate it looks at the frames it is given.  A field with bits 14 and 15 runs the temporal term as well, the
 * encoder's launches.  (av1mi_film_grain_estimate and av1mi_film_grain_ar_estimate accept those bits and behave as without them.) */
int av1mi_film_grain_denoise(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                             const uint8_t *use_table, void *out, uint8_t *table);
/* The same with the temporal term's vectors in the open (AV1MI_FILM_GRAIN_DENOISE_TEMPORAL; AV1MI_E_INVALID_ARG without bits 14 and 15).
 * use_table, out and table as above; out may be NULL when only mv is wanted.  mv (optional, host): n_frames * 4 * nb entries,
 * nb = ceil(coded width / 16) * ceil(coded height / 16) blocks in raster order, at [(f * 4 + slot) * nb + b] the key the filter ran with
 * for frame f, its neighbour g = f - 2, f - 1, f + 1, f + 2 (slot 0 .. 3) and block b: (cost << 11) | index as av1mi_temporal_filter
 * reports its own - index = (dy + R) * (2 R + 1) + (dx + R), R = me_range -, 0xFFFFFFFF where g is no frame of the chunk or beyond the
 * span.  use_mv (optional, host, same layout): the search is skipped and the entries' indexes are taken as they are; 0xFFFFFFFF: the
 * block has no such neighbour; an index of (2 R + 1)^2 or more is AV1MI_E_INVALID_ARG; entries of slots beyond the span or outside
 * the chunk are ignored.  The arguments are checked before a device is touched. */
int av1mi_film_grain_denoise_temporal(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                                      const uint8_t *use_table, const uint32_t *use_mv, void *out, uint8_t *table, uint32_t *mv);

/* ---- the film grain's autoregressive fit on its own --------------------------------------------------
 * What av1mi_encode_chunk runs on a chunk's source when av1mi_params.film_grain carries bit 8 and a lag in bits 12-13
 * (AV1MI_FILM_GRAIN_AR): the estimate's launches and the fit's, on the same frames, taken as one chunk.  Every output is optional, host
 * memory.  coeffs[plane * 25 + i]: the Q7 coefficients in the order the header codes them (rows -L .. 0, columns -L .. L, up to the
 * sample itself), for U and V the luma tap behind them; entries the lag does not use are 0.  table[plane * 8 + k]: what the headers carry,
 * the estimate's value scaled by the plane's gain.  sigma_table: the same before the scaling - what av1mi_film_grain_estimate returns
 * and the denoiser uses.  gain[plane]: Q8, 64 .. 256 (256: no fit).  flat_blocks[plane]: the blocks the sums ran over.
 * sums[plane * 46 + k]: R[dy][dx], the sum of e[r][c] e[r + dy][c + dx] in sixteenths of a sample squared, at k = dx for dy = 0
 * (dx = 0 .. 6) and k = 7 + 13 (dy - 1) + dx + 6 for dy = 1 .. 3 (dx = -6 .. 6); zeros where dy > L or |dx| > 2 L.
 * AV1MI_E_INVALID_ARG without bits 12-13; the arguments are checked before a device is touched.  (av1mi_film_grain_estimate and
 * av1mi_film_grain_denoise accept a field with bits 12-13 and behave as without them: they report the sigma table.) */
int av1mi_film_grain_ar_estimate(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                                 int8_t *coeffs, uint8_t *table, uint8_t *sigma_table, uint32_t *gain, uint32_t *flat_blocks, int64_t *sums);
/* The fit of the context's last successfully encoded chunk, layouts as above, every output optional; zeros, with gains of 256, for a
 * chunk without a lag.  The values arrive with the chunk's other small results.  AV1MI_E_INVALID_ARG without such a chunk. */
int av1mi_film_grain_ar_result(const av1mi_ctx *ctx, int8_t *coeffs, uint8_t *sigma_table, uint32_t *gain);

/* ---- deblocking levels of the last chunk ---------------------------------------------------
 * loop_filter_level[0..3] (luma vertical edges, luma horizontal, U, V) every frame of the context's last successfully encoded
 * chunk was deblocked with: levels[4 * f + i], whatever `deblock` was (all 0 without the filter).  err (optional): with
 * deblock = 2 the level search's table, err[(f * 3 + plane) * 16 + i] = squared error of the plane deblocked at candidate i
 * against the source over the signalled size; zeros without the search.  The values arrive with the chunk's other small
 * results: the call only copies them.  AV1MI_E_INVALID_ARG if n_frames is not the last chunk's frame count. */
int av1mi_lf_search_result(const av1mi_ctx *ctx, uint32_t n_frames, uint8_t *levels, uint64_t *err);

/* ---- self-guided fit of the last chunk ------------------------------------------------------
 * With enable_lr bit 8 (AV1MI_LR_FIT): per restoration unit of the context's last successfully encoded chunk
 * units[((f * 3 + plane) * n_units + u) * 4 + 0..3] = { choice, lr_sgr_set, xqd0, xqd1 } - choice 0 = off, 1..3 = Wiener filter,
 * 4..6 = fixed self-guided candidate, 7 + t = parameter set t with fitted weights (set and weights 0 unless choice >= 4) - and
 * (optional) err[((f * 3 + plane) * n_units + u) * 23 + choice] = the candidates' squared error against the source, UINT64_MAX for
 * an absent candidate (a set outside the mask, or a singular fit).  n_units = unit rows x unit columns of a plane at the chunk's unit
 * size U = 64 << lr_unit_shift (enable_lr bits 12-13), max(1, (size + U / 2) / U) each way from the signalled size; units in raster
 * order, the arrays dense at that count.  Entries are zero for planes that are not restored
 * and for a chunk without the fit.  The values arrive with the chunk's other small results: the call only copies them.
 * AV1MI_E_INVALID_ARG if n_frames is not the last chunk's frame count. */
int av1mi_lr_fit_result(const av1mi_ctx *ctx, uint32_t n_frames, int8_t *units, uint64_t *err);
/* n_units of the context's last successfully encoded chunk, at that chunk's unit size (0: none): what a caller sizes the two arrays above by -
 * units holds n_frames * 3 * n_units * 4 entries, err n_frames * 3 * n_units * 23 */
uint32_t av1mi_lr_fit_units(const av1mi_ctx *ctx);

/* ---- Wiener fit of the last chunk ------------------------------------------------------------
 * With enable_lr bit 10 (AV1MI_LR_WIENER_FIT): per restoration unit of the context's last successfully encoded chunk
 * units[((f * 3 + plane) * n_units + u) * 8 + 0..7] = { final choice 0..23, fitted candidate present, cv0, cv1, cv2, ch0, ch1, ch2 } -
 * choice 23 = the fitted Wiener filter with the vertical taps cv and the horizontal taps ch (tap 0 of a chroma filter is 0), any
 * other value the choice of the decision before the fit (av1mi_lr_fit_result keeps reporting that decision) - and (optional)
 * err[(f * 3 + plane) * n_units + u] = the fitted candidate's squared error against the source, UINT64_MAX if it is absent (a
 * singular fit).  n_units and the unit order are av1mi_lr_fit_result's.  Entries are zero for planes that are not restored and for a
 * chunk without the fit.  The values arrive with the chunk's other small results: the call only copies them.
 * AV1MI_E_INVALID_ARG if n_frames is not the last chunk's frame count. */
int av1mi_lr_wiener_fit_result(const av1mi_ctx *ctx, uint32_t n_frames, int8_t *units, uint64_t *err);
/* n_units of the context's last successfully encoded chunk, at that chunk's unit size (0: none): units holds n_frames * 3 * n_units * 8 entries, err
 * n_frames * 3 * n_units */
uint32_t av1mi_lr_wiener_fit_units(const av1mi_ctx *ctx);

/* ---- restoration decisions of the last chunk --------------------------------------------------
 * For every enable_lr value with a low byte of 1 .. 4, with or without the rate term (AV1MI_LR_RD): per restoration unit of the context's
 * last successfully encoded chunk choice[(f * 3 + plane) * n_units + u] = the unit's final choice 0 .. 23 in av1mi_lr_wiener_fit_result's
 * numbering, (optional) bits16[...] = B16 of that choice - 16 x the length of its coefficients against the plane's tile-start references
 * plus the cost of its type symbol under the default CDFs, in sixteenths of a bit; what the rate term weighs - and (optional)
 * *lambda = the lambda the chunk's decisions used, 0 without the rate term.  n_units (av1mi_lr_rd_units) and the unit order are
 * av1mi_lr_fit_result's.  Entries are zero for planes that are not restored and for a chunk without restoration.  The call reads the
 * choices back from the device.  AV1MI_E_INVALID_ARG if n_frames is not the last chunk's frame count. */
int av1mi_lr_rd_result(const av1mi_ctx *ctx, uint32_t n_frames, int8_t *choice, uint32_t *bits16, uint64_t *lambda);
uint32_t av1mi_lr_rd_units(const av1mi_ctx *ctx);

/* ---- symbolize's tile order of the last chunk ------------------------------------------------
 * An all-key-frame chunk with one-superblock tiles, adaptive CDFs and block_log2 <= 5 is symbolized heavy tiles first (the
 * environment variable AV1MI_SYM_ORDER = 0, read when the context is created, keeps natural order).  A tile's weight is the sum of its
 * transform blocks' eobs, its class 0 .. 15 a monotone step function of the weight (class 0: weight 0).  For the context's last
 * successfully encoded chunk order[0 .. n) = the chunk-wide tile indices (frame * tiles per frame + tile) in the order symbolize took them,
 * a permutation with non-increasing class - the order inside a class differs from run to run, the bytes do not depend on it - and
 * classes[tile] = that tile's class.  n must be av1mi_sym_order_tiles; the call reads the table back from the device.
 * AV1MI_E_INVALID_ARG if the last chunk was symbolized in natural order (av1mi_sym_order_tiles is 0 then) or n is not its tile count. */
int av1mi_sym_order_result(const av1mi_ctx *ctx, uint32_t *order, uint8_t *classes, uint32_t n);
uint32_t av1mi_sym_order_tiles(const av1mi_ctx *ctx);

/* ---- the inter frames' partition of the last chunk ------------------------------------------
 * With partition_search 1 or 2: masks[f * n_sb + sb] = the split mask of superblock sb
 * (raster order, n_sb = ceil(w / 64) * ceil(h / 64)) of frame f of the context's last successfully encoded chunk - bit 0 the 64x64 node,
 * bits 1 .. 4 the 32x32 nodes, bits 5 .. 20 the 16x16 nodes, each level in Z order; the source rule's masks (key frames, and every
 * frame under partition_search = 1) hold a bit for every node the rule would split, an inter frame's under partition_search = 2 only for a
 * node that was reached and decided - and, with partition_search = 2 and inter frames in the chunk (zeros otherwise), keys[f * n_units + u] = the integer search's key at 8x8 unit u
 * (raster order over the coded size): at a leaf's origin unit (centre code << 40) | (cost << 16) | candidate index, UINT64_MAX if the leaf
 * has no valid candidate; other units and key frames are unspecified.  n_units = av1mi_inter_partition_units (0: the last chunk
 * had no partition map).  The call reads both arrays back from the device, where they stand until the context's next chunk.
 * AV1MI_E_INVALID_ARG if n_frames is not that chunk's frame count. */
int av1mi_inter_partition_result(const av1mi_ctx *ctx, uint32_t n_frames, uint32_t *masks, uint64_t *keys);
uint32_t av1mi_inter_partition_units(const av1mi_ctx *ctx);

/* ---- quality: SSIM and exact squared error of one chunk against another, on the device ---------------------------------------
 * The measure is libaom's aom_ssim2 in integers (av1-base_amd/csrc/ssim_rule.h): 8x8 windows at every (4 i, 4 j) of a plane at the
 * signalled size - ny = (h - 8) / 4 + 1 rows of them for h >= 8, else none; nx likewise - each window's value truncated to Q24, so that
 * every implementation agrees bit for bit.  Per frame and plane (chroma (h + 1) / 2 x (w + 1) / 2): sse = sum (a - b)^2 over the whole
 * plane, exact; ssim_sum = the sum of the window values; windows = ny * nx (0 for a plane under 8 samples either way: the chroma of
 * an 8x8 frame).  The SSIM a person reads is ssim_sum / (windows * 2^24), formed by the caller. */
typedef struct { uint64_t sse; int64_t ssim_sum; uint32_t windows; uint32_t reserved; } av1mi_plane_quality;   /* 24 bytes */

/* `test` against `ref`: two chunks of n_frames frames in the callers' layout (tight planar frames as for av1mi_scene_cuts, both host
 * memory or both 16-byte aligned device memory).  Of the parameters only width, height and bit_depth matter.  out[f * 3 + plane]: frame
 * f's plane.  window_map (optional, host memory): per frame, Y then U then V, each plane's ny * nx window values in raster order, dense -
 * n_frames * (the three planes' windows) entries.  Null arguments, n_frames == 0 and misaligned device pointers are
 * AV1MI_E_INVALID_ARG before a device is touched. */
int av1mi_quality(av1mi_ctx *ctx, const av1mi_params *params, const void *ref, const void *test, uint32_t n_frames, int frames_on_device,
                  av1mi_plane_quality *out, int32_t *window_map);
/* The same inside the encoder, default off: with `on` != 0 every chunk the context encodes from then on ends with one more launch, the
 * final reconstruction against the coded source (what av1mi_report.sse is taken against), beside the squared-error launch; the
 * bitstream does not depend on the switch. */
int av1mi_ctx_set_quality(av1mi_ctx *ctx, uint32_t on);
/* out[f * 3 + plane] of the context's last successfully encoded chunk; zeros (windows = 0) for a chunk encoded with the switch off.  The
 * values arrive with the chunk's other small results: the call only copies them.  AV1MI_E_INVALID_ARG without such a chunk or if
 * n_frames is not its frame count. */
int av1mi_quality_result(const av1mi_ctx *ctx, uint32_t n_frames, av1mi_plane_quality *out);

/* ---- film-grain synthesis: what a decoder makes of film_grain_params, on the device ------------------------------------------
 * AV1 spec 7.18.3 for 4:2:0, bit-exact with dav1d (av1-base_amd/csrc/fg_synth_rule.h).  The parameter set
 * is every field of film_grain_params (spec 5.9.30) except grain_seed, coefficients and points as the spec's variables hold them
 * (ar_coeffs_* without the + 128): point_*[k] = { x, y }, x strictly increasing; ar_coeffs_y holds 2 L (L + 1) values at lag L,
 * ar_coeffs_cb / _cr one more, the luma tap.  mc_identity: the sequence's matrix_coefficients is MC_IDENTITY (the chroma maximum of
 * clip_to_restricted_range). */
typedef struct {
  uint8_t num_y_points, num_cb_points, num_cr_points, chroma_scaling_from_luma;   /* at most 14, 10, 10 */
  uint8_t point_y[14][2], point_cb[10][2], point_cr[10][2];
  uint8_t grain_scaling_minus_8, ar_coeff_lag, ar_coeff_shift_minus_6, grain_scale_shift;   /* each 0 .. 3 */
  int8_t ar_coeffs_y[24], ar_coeffs_cb[25], ar_coeffs_cr[25];
  uint8_t overlap_flag, clip_to_restricted_range;
  uint8_t cb_mult, cb_luma_mult, cr_mult, cr_luma_mult;
  uint16_t cb_offset, cr_offset;   /* 0 .. 511 */
  uint8_t mc_identity, reserved[3];
} av1mi_grain_params;   /* 164 bytes */
uint32_t av1mi_grain_params_size(void);   /* sizeof(av1mi_grain_params), for a binding to check its mirror */

/* out = frames with the grain of `g` added: n_frames frames in the layout and residency of av1mi_quality (tight planar frames, both host
 * memory or both 16-byte aligned device memory), of the parameters only width, height and bit_depth - and first_frame where seeds is
 * null - matter.  seeds[f]: frame f's grain_seed; null: the encoder's rule, 7391 + 173 (first_frame + f) mod 65536.  A table with no
 * points and chroma_scaling_from_luma = 0 copies the input.  Null arguments, n_frames == 0, out == frames, more points than a plane
 * may have or points out of order, a lag or shift above 3, an offset above 511 and misaligned device pointers are
 * AV1MI_E_INVALID_ARG before a device is touched. */
int av1mi_film_grain_synth(av1mi_ctx *ctx, const av1mi_params *params, const void *frames, uint32_t n_frames, int frames_on_device,
                           const av1mi_grain_params *g, const uint16_t *seeds, void *out);
/* What the frame headers of the context's last successfully encoded chunk carry, without the seed: the fixed two-point table, or the
 * estimate's eight points (scaled by the fit's gain with a lag), the coefficients, shifts and multipliers - what a decoder of that
 * chunk synthesises with.  AV1MI_E_INVALID_ARG without such a chunk or if it was encoded with film_grain = 0. */
int av1mi_film_grain_params_result(const av1mi_ctx *ctx, av1mi_grain_params *g);
/* The displayed picture's quality inside the encoder, default off: with `on` != 0 every chunk encoded with film_grain != 0 ends with
 * the synthesis of its final reconstruction (the headers' parameters and seeds) into a buffer of the context's, and the quality pass of
 * that against the frames as the caller gave them - not the denoised or temporally filtered ones.  The bitstream, the reconstruction
 * and av1mi_report do not depend on the switch. */
int av1mi_ctx_set_displayed_quality(av1mi_ctx *ctx, uint32_t on);
/* out[f * 3 + plane] of the context's last successfully encoded chunk: zeros for a chunk encoded with the switch off or without film
 * grain.  AV1MI_E_INVALID_ARG without such a chunk or if n_frames is not its frame count. */
int av1mi_displayed_quality_result(const av1mi_ctx *ctx, uint32_t n_frames, av1mi_plane_quality *out);

/* ---- the drop-in for `run_av1an` ---------------------------------------------------------
 * Replaces  pub fn run_av1an(params: &Av1anEncodeParams) -> Result<(), EncodeError>
 * (crates/daemon/src/encode/av1an.rs:126-139), called from JobExecutor::execute through
 * tokio::task::spawn_blocking (crates/daemon/src/job_executor.rs:279-287).
 * Field for field `Av1anEncodeParams` (av1an.rs:36-45): input_path, output_path,
 * temp_chunks_dir, concurrency.av1an_workers. */
typedef struct {
  const char *input_path;   /* Y4M (420jpeg/420p10) - container demux/decode is out of scope */
  const char *output_path;  /* IVF written atomically (tmp + rename); never left zero-length */
  const char *temp_dir;     /* caller-owned scratch (job_executor.rs:275-276); only tmp files go here */
  uint32_t workers;         /* chunks in flight = contexts, placed on the allowed GPUs by av1mi_plan_workers; 0 = default
                               (AV1MI_DEFAULT_WORKERS_PER_GPU per allowed GPU) */
  uint32_t chunk_frames;    /* frames per chunk; 0 = chunks end at detected scene cuts (av1mi_scene_cuts,
                               min scene 12 frames) and after 240 frames at the latest (the reference's
                               `--keyint 240`, av1an.rs:14) */
  int32_t gpu_mask;         /* bit i = may use GPU i; <= 0 = all visible */
  av1mi_params params;      /* width/height/bit_depth are taken from the Y4M header */
} av1mi_job;

/* frames_total: the clip's length when the input is a regular file (from its size), else the frames read so far */
typedef void (*av1mi_progress_cb)(void *user, uint32_t frames_done, uint32_t frames_total, double fps,
                                  uint64_t bytes_out);

/* What the daemon's probe pass (JobMetrics.total_frames / bitrate_kbps, crates/daemon/src/metrics.rs:12-30; zeros today, job_executor.rs:117-137) needs
 * from a Y4M input: geometry, frame rate, range tag, frame count (0 = unknown: not a regular file). */
typedef struct {
  uint32_t width, height, bit_depth, fps_num, fps_den, color_range;
  uint64_t frames;
} av1mi_clip_info;
int av1mi_probe_y4m(const char *path, av1mi_clip_info *info);

int av1mi_encode_file(const av1mi_job *job, av1mi_progress_cb cb, void *user, av1mi_report *total);
/* av1mi_encode_file with the quality switch on in its workers' contexts (they go back to the cache with it off): sum[plane] = the three
 * planes' sse, ssim_sum and windows added up over all frames of all chunks; the output file is the one av1mi_encode_file writes.
 * sum == NULL is av1mi_encode_file. */
int av1mi_encode_file_quality(const av1mi_job *job, av1mi_progress_cb cb, void *user, av1mi_report *total, av1mi_plane_quality sum[3]);

/* av1mi_encode_file keeps its idle contexts (streams + HBM workspace) and pinned host buffers for the next job of the process -
 * the daemon encodes job after job (job_executor.rs:266-437), and setting them up costs more than a short clip's encode.
 * Bounded (8 contexts per GPU, 24 GiB of host buffers); this returns everything that is idle. */
void av1mi_release_caches(void);

/* ---- chunk -> GPU placement (independent chunks, no exchange step) -----------------------------------------
 * Replaces the placement av1an does implicitly by forking `--workers N` encoder processes on one host (av1an.rs:100-101;
 * ConcurrencyPlan.av1an_workers, concurrency.rs:9-18, 67-73).  Two pure functions, so the rule can be tested without a GPU and
 * is the same wherever chunks meet devices (av1mi_encode_file's worker pool, bench.py's ranks):
 *   av1mi_chunk_owner   chunk i of a job -> owner i mod n_owners (owner = a rank of the N-GPU bench, or a GPU of one process)
 *   av1mi_plan_workers  `workers` contexts over the GPUs `gpu_mask` allows among `n_devices`: worker i -> the
 *                       av1mi_chunk_owner(i, allowed)-th allowed device; workers == 0 -> AV1MI_DEFAULT_WORKERS_PER_GPU per allowed
 *                       GPU; at most 64.  Writes min(result, cap) entries; returns the worker count, 0 if no device is allowed. */
#define AV1MI_DEFAULT_WORKERS_PER_GPU 4
uint32_t av1mi_chunk_owner(uint32_t chunk_index, uint32_t n_owners);
int av1mi_plan_workers(uint32_t workers, int32_t gpu_mask, int n_devices, int32_t *device_of_worker, uint32_t cap);

/* ---- the caller's encode segment ---------------------------------------------------------------
 * Mirror of the part of JobExecutor::execute that surrounds the encode call (crates/daemon/src/job_executor.rs:
 * 266-317 and 413-436): state -> "encoding", create `{temp_base_dir}/chunks_{id}`, run the encode, on success state ->
 * "validating" and require the output to exist and be non-empty, remove the chunks directory on every path, and fill the
 * JobMetrics fields the reference leaves at zero (metrics.rs:12-30; job_executor.rs:117-137).  Size gate, atomic
 * replacement and skip markers (job_executor.rs:319-411) stay with the caller: control plane, out of scope.
 * `state_cb` is called with the reference's stage strings ("encoding", "validating", then "size_gating" when the segment
 * hands back to the caller, or "failed"); `error` receives the reference's failure text ("Output file not found: ...",
 * "Output file is empty", "MI355X encoder failed with exit code: N", "IO error: ...").  Returns 0, or the failing code. */
typedef struct {
  const char *id;              /* Job.id */
  const char *input_path, *output_path;
  const char *temp_base_dir;   /* JobExecutor.temp_base_dir */
  uint32_t workers;            /* ConcurrencyPlan.av1an_workers */
  av1mi_params params;
} av1mi_exec_job;

typedef struct {               /* JobMetrics (metrics.rs:12-30), the fields this path can fill */
  char stage[16];
  float progress, fps, bitrate_kbps, psnr;
  uint32_t crf, workers;
  uint64_t frames_encoded, total_frames, size_in_bytes_after;
} av1mi_job_metrics;

typedef void (*av1mi_state_cb)(void *user, const char *stage, const av1mi_job_metrics *m);

int av1mi_job_execute(const av1mi_exec_job *job, av1mi_state_cb state_cb, void *user, av1mi_job_metrics *metrics,
                      char *error, size_t error_cap);

/* Layout pin of this ABI: a binding (integration/mi355x.rs, the ctypes mirror) that was written against another revision of a structure
 * corrupts memory silently - AV1MI_ABI_VERSION is bumped by hand.  Writes up to `cap` entries
 *   { sizeof(av1mi_params), sizeof(av1mi_job), sizeof(av1mi_report), sizeof(av1mi_buf), sizeof(av1mi_clip_info), sizeof(av1mi_scene_state),
 *     sizeof(av1mi_exec_job), sizeof(av1mi_job_metrics), offsetof(av1mi_job, params), offsetof(av1mi_report, ms_h2d),
 *     offsetof(av1mi_exec_job, params), offsetof(av1mi_job_metrics, frames_encoded) }
 * and returns how many there are (12); a binding asserts them against its own `size_of` / `offset_of` once at start-up
 * (integration/mi355x.rs: `check_layout`; tests/test_abi_host.py does it for the ctypes mirror). */
#define AV1MI_LAYOUT_ENTRIES 12
uint32_t av1mi_struct_sizes(uint32_t *sizes, uint32_t cap);

/* helpers shared with the host mirror / tests */
uint32_t av1mi_cq_to_qindex(uint32_t cq_level);
uint32_t av1mi_abi_version(void);
/* writes the sequence header OBU + frame header bytes the encoder will emit (for KATs) */
int av1mi_write_headers(const av1mi_params *p, uint8_t *seq_hdr, size_t *seq_len, uint8_t *frame_hdr,
                        size_t *frame_hdr_bits);

#ifdef __cplusplus
}
#endif
#endif
