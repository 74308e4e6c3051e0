// tpl_rule.h - the temporal-dependency rule of the adaptive quantisation (av1mi_params.cq_level bits 12-14: tpl_strength; DESIGN.md §3
// item 1d), all integers, for host and device: tpl_kernel.hip runs it per 16x16 block, per superblock and per chunk,
// tests/host/tpl_rule_host.cpp compiles it for the CPU against the numpy restatement (tests/tpl_ref.py).  Non-normative, like aq_rule.h:
// the decoder only sees the per-superblock quantiser index.  The frame term (bits 20-22: fq_strength; §3 item 1e) is at the end of the
// file, with tests/host/fq_rule_host.cpp and tests/fq_ref.py.
//
//   block        16x16 luma samples of the coded size, nbx = ceil(cw / 16) by nby = ceil(ch / 16), coordinates clamped to the frame
//   intra cost   S = the sum of the block's 256 samples, m = (S + 128) >> 8, I = max(1, sum |x - m|)
//   inter cost   frames f with f % keyint != 0: the full search of +-me_range whole samples around zero against SOURCE frame f - 1 with
//                me_rule.h's reach, cost SAD + 16 (|dx| + |dy|), index and first-minimum tie break (tf_search.h);
//                C = min(the winner's SAD, I).  Key frames: C = I.  (No pre-search: motion beyond the range gives C ~ I, nothing flows.)
//   flow         A[f][b] = 0; for f from the last frame down, key frames skipped: T = ((I - C) (I + A[f][b])) / I, floored, in 64 bits;
//                the block displaced by its vector overlaps up to four blocks of frame f - 1's grid, each receives (T area) >> 8 into
//                A[f - 1][.]; area outside the grid is dropped.  Nothing flows across a key frame.
//   superblock   O = sum I, P = sum (I + A) over its 16x16 blocks inside the grid; beta = L(P) - L(O) >= 0, L = aq_rule.h's log2 in
//                sixteenths taken to 64-bit arguments
//   chunk        Mb = (sum beta + N / 2) / N over the N superblocks of all frames of the chunk
//   delta        t = aq_strength (E - M) - tpl_strength (beta - Mb); d from t as aq_rule.h makes it, clamp included; index base + 4 d
#ifndef AV1MI_TPL_RULE_H
#define AV1MI_TPL_RULE_H
#include <stddef.h>
#include <stdint.h>
#include "aq_rule.h"

#define AV1MI_TPL_MAX_STRENGTH 4
#define AV1MI_TPL_BLOCK 16

// the blocks of an axis of `size` samples
AV1MI_AQ_HD inline int av1mi_tpl_blocks(int size) { return (size + AV1MI_TPL_BLOCK - 1) / AV1MI_TPL_BLOCK; }
// the entries of a chunk's flow buffer: A per [frame][block] of the coded size w x h, and behind them the chunk's sum of beta - one fill
// clears both
AV1MI_AQ_HD inline size_t av1mi_tpl_flow_entries(int w, int h, int n_frames) {
  return (size_t)n_frames * (size_t)av1mi_tpl_blocks(w) * (size_t)av1mi_tpl_blocks(h) + 1;
}

// m and I of a block from its sum S and, once m is known, from D = sum |x - m|
AV1MI_AQ_HD inline uint32_t av1mi_tpl_mean(uint32_t S) { return (S + 128u) >> 8; }
AV1MI_AQ_HD inline uint32_t av1mi_tpl_intra(uint32_t D) { return D < 1u ? 1u : D; }
// C of an inter block from the winner's SAD
AV1MI_AQ_HD inline uint32_t av1mi_tpl_inter(uint32_t sad, uint32_t I) { return sad < I ? sad : I; }

// L on 64-bit arguments, x >= 1: equal to av1mi_aq_log2_q4 wherever that is defined
AV1MI_AQ_HD inline int av1mi_tpl_log2_q4(uint64_t x) {
  const int k = 63 - __builtin_clzll(x);
  return 16 * k + (int)((k >= 4 ? x >> (k - 4) : x << (4 - k)) & 15u);
}

// T of a block: what it hands to the frame before it
AV1MI_AQ_HD inline uint64_t av1mi_tpl_flow(uint32_t I, uint32_t C, uint64_t A) { return ((uint64_t)(I - C) * ((uint64_t)I + A)) / I; }

// Part k = 0 .. 3 of the split of T: block (bx, by) displaced by (dx, dy) whole samples covers the cells (gx + (k & 1), gy + (k >> 1)) of the
// grid of nbx x nby blocks, gx = floor((16 bx + dx) / 16), likewise gy.  Returns the cell's raster index, or -1 for a part without area
// or outside the grid; *share = (T area) >> 8.
AV1MI_AQ_HD inline int av1mi_tpl_part(int k, int bx, int by, int dx, int dy, int nbx, int nby, uint64_t T, uint64_t *share) {
  const int px = bx * AV1MI_TPL_BLOCK + dx, py = by * AV1MI_TPL_BLOCK + dy;
  const int ox = px & 15, oy = py & 15;                                  // (two's complement: the floor's remainder)
  const int cx = (px >> 4) + (k & 1), cy = (py >> 4) + (k >> 1);         // (arithmetic shifts: the floor)
  const int w = (k & 1) ? ox : 16 - ox, h = (k >> 1) ? oy : 16 - oy;
  *share = (T * (uint64_t)(w * h)) >> 8;
  return w * h == 0 || cx < 0 || cy < 0 || cx >= nbx || cy >= nby ? -1 : cy * nbx + cx;
}

// beta of a superblock from O = sum I and P = sum (I + A)
AV1MI_AQ_HD inline int av1mi_tpl_beta(uint64_t O, uint64_t P) { return av1mi_tpl_log2_q4(P) - av1mi_tpl_log2_q4(O); }
// Mb of a chunk from the sum over its N superblocks
AV1MI_AQ_HD inline int av1mi_tpl_mean_beta(uint64_t sum, uint64_t N) { return (int)((sum + N / 2) / N); }

// d and the index of a superblock with both terms (either strength may be 0)
AV1MI_AQ_HD inline int av1mi_tpl_delta(int aq_strength, int E, int M, int tpl_strength, int beta, int Mb, int base) {
  return av1mi_aq_delta_of(aq_strength * (E - M) - tpl_strength * (beta - Mb), base);
}
AV1MI_AQ_HD inline int av1mi_tpl_qindex_of(int aq_strength, int E, int M, int tpl_strength, int beta, int Mb, int base) {
  return base + 4 * av1mi_tpl_delta(aq_strength, E, M, tpl_strength, beta, Mb, base);
}

// ---- the frame term (av1mi_params.cq_level bits 20-22: fq_strength): every frame of the chunk gets a base_q_idx
// of its own from the same analysis.  Non-normative like the rest: the decoder reads the index from the frame's header.
//   frame        OF = sum I, PF = sum (I + A) over all nbx nby blocks of the frame, 64 bits; betaF = L(PF) - L(OF) >= 0
//   chunk        MF = (sum betaF + n / 2) / n over its n frames
//   step         t = fq_strength (betaF - MF), a = (|t| + 8) >> 4, k = -a for t > 0, else +a; clamped to [AV1MI_FQ_MIN_STEP,
//                AV1MI_FQ_MAX_STEP], then to [-((base - 1) / 4), (255 - base) / 4]; q_f = base + 4 k - strength 1 is one step of 4 per
//                doubling of PF / OF against the chunk's mean
//   superblock   with a spatial or temporal strength as well: the temporal term against the FRAME's mean Mb_f = (sum beta + N / 2) / N
//                over the frame's N superblocks (the frame term moves the frame, the superblock term redistributes inside it);
//                d clamped against q_f, index q_f + 4 d
#define AV1MI_FQ_MAX_STRENGTH 4
#define AV1MI_FQ_MIN_STEP (-10)
#define AV1MI_FQ_MAX_STEP 4

// betaF of a frame from OF = sum I and PF = sum (I + A), OF >= 1
AV1MI_AQ_HD inline int av1mi_fq_beta(uint64_t OF, uint64_t PF) { return av1mi_tpl_log2_q4(PF) - av1mi_tpl_log2_q4(OF); }
// MF of a chunk from the sum over its n frames
AV1MI_AQ_HD inline int av1mi_fq_mean(uint64_t sum, uint64_t n) { return (int)((sum + n / 2) / n); }
// k_f and q_f of a frame
AV1MI_AQ_HD inline int av1mi_fq_step(int fq_strength, int betaF, int MF, int base) {
  const int t = fq_strength * (betaF - MF), a = ((t < 0 ? -t : t) + 8) >> 4;
  int k = t > 0 ? -a : a;
  k = k < AV1MI_FQ_MIN_STEP ? AV1MI_FQ_MIN_STEP : (k > AV1MI_FQ_MAX_STEP ? AV1MI_FQ_MAX_STEP : k);
  const int lo = -((base - 1) / 4), hi = (255 - base) / 4;
  return k < lo ? lo : (k > hi ? hi : k);
}
AV1MI_AQ_HD inline int av1mi_fq_qindex(int fq_strength, int betaF, int MF, int base) { return base + 4 * av1mi_fq_step(fq_strength, betaF, MF, base); }
// the index of a superblock of a frame coded at q_f: av1mi_tpl_qindex_of with the frame's mean and the frame's index
AV1MI_AQ_HD inline int av1mi_fq_sb_qindex(int aq_strength, int E, int M, int tpl_strength, int beta, int Mb_f, int q_f) {
  return av1mi_tpl_qindex_of(aq_strength, E, M, tpl_strength, beta, Mb_f, q_f);
}

#endif
