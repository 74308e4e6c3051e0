// The CDEF pieces (av1-base_amd/csrc/cdef_pieces.h) compiled for the host: tests/test_cdef_search_host.py checks the whole-frame
// loop over them against oracle/av1o_cdef.c, the strength search's 24 errors per superblock against oracle runs at fixed strengths,
// and the candidate pool against a Python restatement.
// With -DCDEF_PIECES_MAIN the file is a program of its own: random frames and skip maps at the test's sizes - built with
// -fsanitize=address,undefined it checks that no tap load leaves its plane; it also checks that the search's errors are the squared
// errors of the filter run at each candidate's strengths.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../av1-base_amd/csrc/cdef_pieces.h"

namespace {
struct Frame {
  const uint16_t *pl[3];
  int w, h, bd, damping;     // coded luma size (multiples of 8), 4:2:0, tight planes
  const uint8_t *skip8;      // per 8x8 luma block
  int b8_cols() const { return w / 8; }
};
// cdef_sb_kernel's edge rule: taps reach 2 samples beyond the superblock; interior superblocks load without tests
bool sb_edge(const Frame &F, int x0, int y0) { return x0 < 2 || y0 < 2 || x0 + 66 > F.w || y0 + 66 > F.h; }

// one 8x8 block (4x4 in chroma) of one plane through the sample filter, as cdef_rows runs it: strengths 0 where the block is off,
// NT = 12 taps where the plane has a secondary strength, else the 4 primary taps
template <bool EDGE, int NT>
void filter_block(const Frame &F, int plane, int bx, int by, bool on, int pri, int sec, int dir, uint16_t *out) {
  const int ss = plane > 0, pw = F.w >> ss, ph = F.h >> ss, n = 8 >> ss, coeff_shift = F.bd - 8;
  const int damping = F.damping + coeff_shift - ss;
  if (!on) pri = sec = 0;
  const int pri_shift = av1mi_cdef_damp_shift(pri, damping), sec_shift = av1mi_cdef_damp_shift(sec, damping);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const int gy = by * n + i, gx = bx * n + j;
      const int x = av1mi_cdef_ld(F.pl[plane], gy * pw + gx);
      int t[NT];
      av1mi_cdef_load_taps<uint16_t, EDGE, NT>(F.pl[plane], pw, pw, ph, gy, gx, dir, x, t);
      out[(size_t)gy * pw + gx] = (uint16_t)av1mi_cdef_sample<NT>(x, t, ~0u, pri, pri_shift, sec, sec_shift, (pri >> coeff_shift) & 1);
    }
}
}  // namespace

// CDEF of a frame of three tight planes (w x h coded luma, 4:2:0) through the pieces: per 8x8 block the direction search, the adjusted
// luma strength and the sample filter.  idx_sb: per superblock -1 (nothing coded: nothing is filtered) or 0.
extern "C" void cdef_frame(const uint16_t *y, const uint16_t *u, const uint16_t *v, uint16_t *oy, uint16_t *ou, uint16_t *ov, int w, int h, int bit_depth,
                           int damping, int y_pri, int y_sec, int uv_pri, int uv_sec, const uint8_t *skip8, const int8_t *idx_sb) {
  const Frame F = { { y, u, v }, w, h, bit_depth, damping, skip8 };
  uint16_t *out[3] = { oy, ou, ov };
  const int coeff_shift = bit_depth - 8, sb_cols = (w + 63) / 64;
  for (int by = 0; by < h / 8; by++)
    for (int bx = 0; bx < w / 8; bx++) {
      const bool on = idx_sb[(by / 8) * sb_cols + bx / 8] >= 0 && !skip8[by * F.b8_cols() + bx];
      int ydir = 0, var = 0;
      if (on) av1mi_cdef_block_direction(y + (size_t)by * 8 * w + bx * 8, w, coeff_shift, ydir, var);
      const bool edge = sb_edge(F, bx / 8 * 64, by / 8 * 64);
      for (int plane = 0; plane < 3; plane++) {
        const int pri = plane ? uv_pri << coeff_shift : av1mi_cdef_adjusted_pri(y_pri, var, coeff_shift);
        const int sec = av1mi_cdef_sec_strength(plane ? uv_sec : y_sec, coeff_shift);
        const int dir = (plane ? uv_pri : y_pri) == 0 ? 0 : ydir;
        if (edge && sec) filter_block<true, 12>(F, plane, bx, by, on, pri, sec, dir, out[plane]);
        else if (edge) filter_block<true, 4>(F, plane, bx, by, on, pri, 0, dir, out[plane]);
        else if (sec) filter_block<false, 12>(F, plane, bx, by, on, pri, sec, dir, out[plane]);
        else filter_block<false, 4>(F, plane, bx, by, on, pri, 0, dir, out[plane]);
      }
    }
}

// The strength search's table as cdef_search_kernel forms it: per superblock 16 luma and 8 chroma (U + V) candidates' squared errors
// against the source over the signalled size (true_w x true_h), from av1mi_cdef_search_luma / _chroma; blocks that are off add their
// unfiltered error to every candidate.  Superblocks with nothing coded: idx_sb -1 and errors 0 (else idx_sb 0).
extern "C" void cdef_search_errors(const uint16_t *y, const uint16_t *u, const uint16_t *v, const uint16_t *sy, const uint16_t *su, const uint16_t *sv,
                                   int w, int h, int true_w, int true_h, int bit_depth, int damping, const uint8_t *skip8,
                                   unsigned long long *err, int8_t *idx_sb) {
  const Frame F = { { y, u, v }, w, h, bit_depth, damping, skip8 };
  const uint16_t *src[3] = { sy, su, sv };
  const int coeff_shift = bit_depth - 8, sb_cols = (w + 63) / 64, sb_rows = (h + 63) / 64;
  for (int i = 0; i < sb_rows * sb_cols; i++) idx_sb[i] = -1;
  memset(err, 0, sizeof(unsigned long long) * 24 * sb_rows * sb_cols);
  for (int i = 0; i < (h / 8) * (w / 8); i++)
    if (!skip8[i]) idx_sb[(i / (w / 8) / 8) * sb_cols + i % (w / 8) / 8] = 0;
  for (int by = 0; by < h / 8; by++)
    for (int bx = 0; bx < w / 8; bx++) {
      const int sb = (by / 8) * sb_cols + bx / 8;
      if (idx_sb[sb] < 0) continue;
      const bool on = !skip8[by * F.b8_cols() + bx], edge = sb_edge(F, bx / 8 * 64, by / 8 * 64);
      int ydir = 0, var = 0;
      if (on) av1mi_cdef_block_direction(y + (size_t)by * 8 * w + bx * 8, w, coeff_shift, ydir, var);
      for (int plane = 0; plane < 3; plane++) {
        const int ss = plane > 0, pw = w >> ss, ph = h >> ss, n = 8 >> ss, nc = ss ? 8 : 16;
        unsigned long long *e = err + (size_t)sb * 24 + (ss ? 16 : 0);
        for (int i = 0; i < n; i++)
          for (int j = 0; j < n; j++) {
            const int gy = by * n + i, gx = bx * n + j;
            if (gx >= (true_w >> ss) || gy >= (true_h >> ss)) continue;
            const int x = F.pl[plane][(size_t)gy * pw + gx], s = src[plane][(size_t)gy * pw + gx];
            int val[16];
            for (int k = 0; k < 16; k++) val[k] = x;
            if (on && !ss) {
              if (edge) av1mi_cdef_search_luma<uint16_t, true>(y, pw, pw, ph, gy, gx, x, ydir, var, coeff_shift, damping + coeff_shift, val);
              else av1mi_cdef_search_luma<uint16_t, false>(y, pw, pw, ph, gy, gx, x, ydir, var, coeff_shift, damping + coeff_shift, val);
            } else if (on) {
              int v8[8];
              if (edge) av1mi_cdef_search_chroma<uint16_t, true>(F.pl[plane], pw, pw, ph, gy, gx, x, ydir, coeff_shift, damping + coeff_shift - 1, v8);
              else av1mi_cdef_search_chroma<uint16_t, false>(F.pl[plane], pw, pw, ph, gy, gx, x, ydir, coeff_shift, damping + coeff_shift - 1, v8);
              for (int k = 0; k < 8; k++) val[k] = v8[k];
            }
            for (int k = 0; k < nc; k++) e[k] += (unsigned long long)((val[k] - s) * (val[k] - s));
          }
      }
    }
}

// the pool: pair -> the header's four strength fields and their 12 bits; a superblock's error under a pair
extern "C" void cdef_pair_strengths(int p, int *out4) {
  const Av1miCdefStrengths s = av1mi_cdef_pair_strengths(p);
  out4[0] = s.y_pri; out4[1] = s.y_sec; out4[2] = s.uv_pri; out4[3] = s.uv_sec;
}
extern "C" unsigned cdef_pair_bits(int p) { return av1mi_cdef_pair_bits(p); }
extern "C" unsigned long long cdef_pair_err(const unsigned long long *e, int p) { return av1mi_cdef_pair_err(e, p); }

#ifdef CDEF_PIECES_MAIN
namespace {
uint32_t rng_state = 4321;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
}  // namespace

// Every luma candidate l and chroma candidate l mod 8 as a fixed-strength run of cdef_frame: the squared error of its output per
// superblock must be the search's table entry.
int main() {
  static const int sizes[][4] = { { 8, 8, 8, 8 }, { 72, 56, 72, 56 }, { 200, 136, 200, 136 }, { 208, 128, 202, 122 } };
  long bad = 0, runs = 0, moved = 0;
  for (const auto &sz : sizes)
    for (int bd = 8; bd <= 10; bd += 2)
      for (int damping = 3; damping <= 6; damping += 3) {
        const int w = sz[0], h = sz[1], tw = sz[2], th = sz[3], sb_cols = (w + 63) / 64, nsb = sb_cols * ((h + 63) / 64);
        std::vector<uint16_t> p[3], s[3], o[3];
        const int mid = 1 << (bd - 1), amp = 12 << (bd - 8);
        for (int pl = 0; pl < 3; pl++) {
          const size_t n = (size_t)w * h >> (pl ? 2 : 0);
          p[pl].resize(n); s[pl].resize(n); o[pl].resize(n);
          const int pw = pl ? w / 2 : w;
          for (size_t i = 0; i < n; i++) {   // diagonal stripes with noise: directions are found and the filters act
            const int gx = (int)(i % pw), gy = (int)(i / pw);
            s[pl][i] = (uint16_t)(mid + (((gx + gy) >> 2) & 1 ? amp : -amp));
            p[pl][i] = (uint16_t)(s[pl][i] + (int)(rnd() % (unsigned)amp) - amp / 2);
          }
        }
        std::vector<uint8_t> skip8((size_t)(w / 8) * (h / 8));
        for (auto &k : skip8) k = (rnd() & 3) == 0;
        if (nsb > 1)
          for (int by = 0; by < 8 && by < h / 8; by++)
            for (int bx = 0; bx < 8; bx++) skip8[(size_t)by * (w / 8) + bx] = 1;   // superblock 0: nothing coded
        std::vector<unsigned long long> err((size_t)nsb * 24);
        std::vector<int8_t> idx(nsb);
        cdef_search_errors(p[0].data(), p[1].data(), p[2].data(), s[0].data(), s[1].data(), s[2].data(), w, h, tw, th, bd, damping, skip8.data(),
                           err.data(), idx.data());
        if (nsb > 1 && idx[0] != -1) bad++;
        for (int l = 0; l < 16; l++) {
          const Av1miCdefStrengths st = av1mi_cdef_pair_strengths(8 * l + (l & 7));
          cdef_frame(p[0].data(), p[1].data(), p[2].data(), o[0].data(), o[1].data(), o[2].data(), w, h, bd, damping, st.y_pri, st.y_sec, st.uv_pri,
                     st.uv_sec, skip8.data(), idx.data());
          runs++;
          std::vector<unsigned long long> ey(nsb, 0), ec(nsb, 0);
          for (int pl = 0; pl < 3; pl++) {
            const int ss = pl > 0, pw = w >> ss;
            for (int gy = 0; gy < (th >> ss); gy++)
              for (int gx = 0; gx < (tw >> ss); gx++) {
                const size_t i = (size_t)gy * pw + gx;
                const long d = (long)o[pl][i] - s[pl][i];
                (ss ? ec : ey)[(gy >> (6 - ss)) * sb_cols + (gx >> (6 - ss))] += (unsigned long long)(d * d);
                moved += o[pl][i] != p[pl][i];
              }
          }
          for (int sb = 0; sb < nsb; sb++) {
            if (idx[sb] < 0) { bad += err[(size_t)sb * 24 + l] != 0; continue; }
            bad += ey[sb] != err[(size_t)sb * 24 + l];
            bad += ec[sb] != err[(size_t)sb * 24 + 16 + (l & 7)];
            bad += cdef_pair_err(err.data() + (size_t)sb * 24, 8 * l + (l & 7)) != ey[sb] + ec[sb];
          }
        }
      }
  int f[4];
  cdef_pair_strengths(127, f);
  if (f[0] != 11 || f[1] != 2 || f[2] != 11 || f[3] != 0 || cdef_pair_bits(127) != ((11u << 8) | (2u << 6) | (11u << 2))) bad++;
  printf("cdef pieces: %ld runs, %ld samples moved, %ld mismatches\n", runs, moved, bad);
  return bad || moved < 1000 ? 1 : 0;
}
#endif
