// The film-grain synthesis rule (av1-base_amd/csrc/fg_synth_rule.h: what fg_synth_kernel.hip runs) compiled for the host, for
// tests/test_fg_synth_host.py - a stand-alone program: reads cases from a text file, one per line, and prints one line of results each.
//   F bd w h seed params frame    a frame: params the 164 bytes of av1mi_grain_params, frame the tight planar frame's bytes, both in hex;
//                                 prints the frame with its grain in hex
//   T bd seed params              the three templates: 9330 values
//   V params                      whether av1mi_film_grain_synth accepts the parameter set: 1 or 0
//   H N estimate lag table coeffs what the encoder's frame headers carry: table the 24 values, coeffs the 75 coefficients, both in hex;
//                                 prints the 164 bytes of the parameter set in hex
//   G                             the Gaussian table's 4096 little-endian bytes in hex
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../av1-base_amd/csrc/fg_synth_rule.h"

static bool read_hex(FILE *f, std::vector<uint8_t> &out) {
  int c;
  do c = fgetc(f); while (c == ' ');
  out.clear();
  auto nib = [](int ch) { return ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1); };
  while (nib(c) >= 0) {
    const int d = fgetc(f);
    if (nib(d) < 0) return false;
    out.push_back((uint8_t)(nib(c) << 4 | nib(d)));
    c = fgetc(f);
  }
  if (c != EOF) ungetc(c, f);
  return true;
}
static void print_hex(const uint8_t *p, size_t n) {
  std::string s(n * 2, '0');
  for (size_t i = 0; i < n; i++) { s[2 * i] = "0123456789abcdef"[p[i] >> 4]; s[2 * i + 1] = "0123456789abcdef"[p[i] & 15]; }
  puts(s.c_str());
}
static bool read_params(FILE *f, av1mi_grain_params &g) {
  std::vector<uint8_t> b;
  if (!read_hex(f, b) || b.size() != sizeof(g)) return false;
  memcpy(&g, b.data(), sizeof(g));
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char t;
  long line = 0;
  int rc = 0;
  while (!rc && fscanf(f, " %c", &t) == 1) {
    av1mi_grain_params g;
    int bd = 0, w = 0, h = 0;
    unsigned seed = 0;
    if (t == 'F') {
      std::vector<uint8_t> in;
      if (fscanf(f, "%d %d %d %u", &bd, &w, &h, &seed) != 4 || !read_params(f, g) || !read_hex(f, in)) rc = 2;
      const size_t n = (size_t)w * h * 3 / 2, bytes = n * (bd > 8 ? 2 : 1);
      if (!rc && (in.size() != bytes || !av1mi_fgs_params_valid(g) || (w & 1) || (h & 1))) rc = 2;
      if (rc) break;
      std::vector<int16_t> tmpl(AV1MI_FGS_TEMPLATE_N);
      std::vector<uint8_t> offs((size_t)av1mi_fgs_stripes(h) * av1mi_fgs_blocks(w)), out(bytes);
      if (bd > 8) {
        std::vector<uint16_t> a(n), b(n);
        memcpy(a.data(), in.data(), bytes);
        av1mi_fgs_frame(g, bd, seed, a.data(), b.data(), w, h, tmpl.data(), offs.data());
        memcpy(out.data(), b.data(), bytes);
      } else {
        av1mi_fgs_frame(g, bd, seed, in.data(), out.data(), w, h, tmpl.data(), offs.data());
      }
      print_hex(out.data(), bytes);
    } else if (t == 'T') {
      if (fscanf(f, "%d %u", &bd, &seed) != 2 || !read_params(f, g)) { rc = 2; break; }
      std::vector<int16_t> tmpl(AV1MI_FGS_TEMPLATE_N);
      av1mi_fgs_templates(g, bd, seed, tmpl.data());
      for (size_t i = 0; i < tmpl.size(); i++) printf(i + 1 < tmpl.size() ? "%d " : "%d\n", tmpl[i]);
    } else if (t == 'V') {
      if (!read_params(f, g)) { rc = 2; break; }
      printf("%d\n", av1mi_fgs_params_valid(g) ? 1 : 0);
    } else if (t == 'H') {
      int N = 0, estimate = 0, lag = 0;
      std::vector<uint8_t> table, coeffs;
      if (fscanf(f, "%d %d %d", &N, &estimate, &lag) != 3 || !read_hex(f, table) || !read_hex(f, coeffs) || table.size() != 24 || coeffs.size() != 75) { rc = 2; break; }
      av1mi_fgs_header_params(N, estimate, lag, table.data(), reinterpret_cast<const int8_t *>(coeffs.data()), &g);
      print_hex(reinterpret_cast<const uint8_t *>(&g), sizeof(g));
    } else if (t == 'G') {
      uint8_t b[2 * AV1MI_FG_GAUSS_N];
      for (int i = 0; i < AV1MI_FG_GAUSS_N; i++) { b[2 * i] = (uint8_t)(av1mi_fg_gaussian_sequence[i] & 0xFF); b[2 * i + 1] = (uint8_t)((av1mi_fg_gaussian_sequence[i] >> 8) & 0xFF); }
      print_hex(b, sizeof(b));
    } else {
      rc = 2;
    }
    line++;
  }
  if (rc) fprintf(stderr, "line %ld: malformed case\n", line);
  fclose(f);
  return rc;
}
