// av1mi_container.cpp - av1mi_encode_file's input and output formats, and av1mi_probe_y4m.  Input is Y4M (demux / decode via ffmpeg is out
// of scope); output is Matroska (.mkv/.webm, the reference's job output `{temp_output_dir}/{uuid}.mkv`, jobs.rs:187-188,
// there muxed by av1an/mkvmerge), IVF or a bare OBU stream.  No HIP header: the counterpart of av1mi_syntax.cpp on the file side.
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <thread>

#include "av1mi_container.h"

namespace av1mi {

int y4m_open(const char *path, Y4m *y) {
  y->f = fopen(path, "rb");
  if (!y->f) return -errno;
  char line[512];
  size_t n = 0;
  int ch;
  while ((ch = fgetc(y->f)) != EOF && ch != '\n' && n < sizeof(line) - 1) line[n++] = (char)ch;
  line[n] = 0;
  if (strncmp(line, "YUV4MPEG2", 9) != 0) return AV1MI_E_FORMAT;
  bool ok420 = true;
  for (char *tok = strtok(line + 9, " "); tok; tok = strtok(nullptr, " ")) {
    switch (tok[0]) {
      case 'W': y->w = (uint32_t)atoi(tok + 1); break;
      case 'H': y->h = (uint32_t)atoi(tok + 1); break;
      case 'F': sscanf(tok + 1, "%u:%u", &y->fps_n, &y->fps_d); break;
      case 'X':
        if (!strcmp(tok, "XCOLORRANGE=FULL")) y->color_range = 1;
        else if (!strcmp(tok, "XCOLORRANGE=LIMITED")) y->color_range = 0;
        break;
      case 'C':
        if (strncmp(tok + 1, "420p10", 6) == 0) y->bd = 10;
        else if (strncmp(tok + 1, "420", 3) == 0 && (tok[4] == 0 || tok[4] == 'j' || tok[4] == 'm' || (tok[4] == 'p' && tok[5] == 'a'))) y->bd = 8;
        else ok420 = false;
        break;
      default: break;
    }
  }
  if (!ok420 || !y->w || !y->h) return AV1MI_E_FORMAT;
  if (!y->fps_n || !y->fps_d) { y->fps_n = 30; y->fps_d = 1; }
  y->frame_bytes = (size_t)y->w * y->h * 3 / 2 * (y->bd > 8 ? 2 : 1);
  {  // frame count of a regular file: every frame is "FRAME\n" + frame_bytes (frame parameters would only make this an over-estimate)
    const long pos = ftell(y->f);
    struct stat sb;
    if (pos >= 0 && fstat(fileno(y->f), &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > pos) {
      // the parallel reader knows where every frame starts only if the markers are the plain six bytes; a clip whose first marker
      // carries frame parameters ("FRAME Ixx\n") goes through the sequential reader, frame count unknown
      char mark[6];
      const bool plain = pread(fileno(y->f), mark, 6, (off_t)pos) == 6 && memcmp(mark, "FRAME\n", 6) == 0;
      if (plain) {
        y->total_frames = (uint64_t)(sb.st_size - pos) / (6 + y->frame_bytes);
        y->data_off = pos;
        y->regular = true;
      }
    }
  }
  return 0;
}

int y4m_read_frame(Y4m *y, uint8_t *dst) {
  char hdr[128];
  size_t n = 0;
  int ch;
  while ((ch = fgetc(y->f)) != EOF && ch != '\n' && n < sizeof(hdr) - 1) hdr[n++] = (char)ch;
  if (ch == EOF && n == 0) return 0;
  hdr[n] = 0;
  if (strncmp(hdr, "FRAME", 5) != 0) return AV1MI_E_FORMAT;
  if (fread(dst, 1, y->frame_bytes, y->f) != y->frame_bytes) return AV1MI_E_FORMAT;
  return 1;
}

// Regular files: the frames sit at known offsets, so up to `threads` readers pread() them in parallel - one thread copies page cache to
// the destination at a few GB/s, which at 6 MB per 1080p 10-bit frame is ~1 k frames/s, a tenth of what one GPU encodes.  Pipes, and
// clips whose markers carry frame parameters: sequential fread.
uint32_t y4m_read_frames(Y4m *y, uint8_t *dst, uint32_t count, int threads, int *err) {
  *err = 0;
  if (!y->regular) {
    uint32_t n = 0;
    int r = 1;
    while (n < count && (r = y4m_read_frame(y, dst + (size_t)n * y->frame_bytes)) == 1) n++;
    if (r != 0 && r != 1) *err = r;
    return n;
  }
  const uint64_t left = y->total_frames > y->next_frame ? y->total_frames - y->next_frame : 0;
  uint32_t n = (uint32_t)(left < count ? left : count);
  if (n == 0) {   // a trailing partial frame is a malformed file, not a clean end
    struct stat sb;
    if (fstat(fileno(y->f), &sb) == 0 && (uint64_t)sb.st_size > (uint64_t)y->data_off + y->next_frame * (6 + y->frame_bytes)) *err = AV1MI_E_FORMAT;
    return 0;
  }
  const int fd = fileno(y->f);
  const uint64_t first = y->next_frame;
  std::atomic<uint32_t> next(0);
  std::atomic<int> bad(0);
  auto work = [&] {
    for (;;) {
      const uint32_t k = next.fetch_add(1);
      if (k >= n || bad.load()) return;
      const off_t off = (off_t)((uint64_t)y->data_off + (first + k) * (6 + y->frame_bytes));
      char mark[6];
      if (pread(fd, mark, 6, off) != 6 || memcmp(mark, "FRAME\n", 6) != 0) { bad.store(AV1MI_E_FORMAT); return; }   // frame parameters are not supported
      uint8_t *d = dst + (size_t)k * y->frame_bytes;
      size_t got = 0;
      while (got < y->frame_bytes) {
        const ssize_t r = pread(fd, d + got, y->frame_bytes - got, off + 6 + (off_t)got);
        if (r <= 0) { bad.store(r < 0 ? -errno : AV1MI_E_FORMAT); return; }
        got += (size_t)r;
      }
    }
  };
  const int nt = threads < 1 ? 1 : ((uint32_t)threads > n ? (int)n : threads);
  std::vector<std::thread> th;
  for (int i = 1; i < nt; i++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  if (bad.load()) { *err = bad.load(); return 0; }
  y->next_frame += n;
  // a clip whose size is not a whole number of frames: the tail shows up as an error once the whole frames are consumed
  return n;
}

void put_le(uint8_t *p, uint64_t v, int n) { for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i)); }

// ---- EBML: IDs as they are written, sizes always in the 8-byte form ------------------------------------------------------------------
namespace {
typedef std::vector<uint8_t> Bytes;
void ebml_id(Bytes &v, uint32_t id) { for (int sh = 24; sh >= 0; sh -= 8) if (id >> sh) v.push_back((uint8_t)(id >> sh)); }
void ebml_size(Bytes &v, uint64_t n) {  // 0x01 + 56 bits
  v.push_back(0x01);
  for (int sh = 48; sh >= 0; sh -= 8) v.push_back((uint8_t)(n >> sh));
}
void ebml_elem(Bytes &v, uint32_t id, const Bytes &payload) { ebml_id(v, id); ebml_size(v, payload.size()); v.insert(v.end(), payload.begin(), payload.end()); }
Bytes be(uint64_t x, int n) { Bytes v; for (int i = n - 1; i >= 0; i--) v.push_back((uint8_t)(x >> (8 * i))); return v; }
Bytes str(const char *s) { return Bytes(s, s + strlen(s)); }
bool ends_with(const char *path, const char *ext) { const char *dot = strrchr(path, '.'); return dot && !strcmp(dot, ext); }
}  // namespace

Muxer::Muxer(FILE *out, const char *output_path, const Y4m &clip, const av1mi_params &prm)
    : fo(out), kind(ends_with(output_path, ".mkv") || ends_with(output_path, ".webm") ? MKV : (ends_with(output_path, ".obu") ? OBU : IVF)),
      webm(ends_with(output_path, ".webm")), w(clip.w), h(clip.h), fps_n(clip.fps_n), fps_d(clip.fps_d), bit_depth(clip.bd),
      cp(prm.color_primaries), tc(prm.transfer_characteristics), mc(prm.matrix_coefficients), full_range(prm.color_range != 0) {}

void Muxer::begin(const Bytes &seq_hdr_obu) {
  if (kind == IVF) {
    uint8_t ivf[32] = { 'D', 'K', 'I', 'F', 0, 0, 32, 0, 'A', 'V', '0', '1' };
    put_le(ivf + 12, w, 2); put_le(ivf + 14, h, 2); put_le(ivf + 16, fps_n, 4); put_le(ivf + 20, fps_d, 4);
    fwrite(ivf, 1, 32, fo);
    bytes = 32;
  } else if (kind == MKV) {
    Bytes hdr, e;
    ebml_elem(e, 0x4286, be(1, 1)); ebml_elem(e, 0x42F7, be(1, 1)); ebml_elem(e, 0x42F2, be(4, 1)); ebml_elem(e, 0x42F3, be(8, 1));
    ebml_elem(e, 0x4282, str(webm ? "webm" : "matroska")); ebml_elem(e, 0x4287, be(4, 1)); ebml_elem(e, 0x4285, be(2, 1));
    ebml_elem(hdr, 0x1A45DFA3, e);
    ebml_id(hdr, 0x18538067);  // Segment, size patched at the end
    fwrite(hdr.data(), 1, hdr.size(), fo);
    seg_size_pos = ftell(fo);
    uint8_t unk[8] = { 0x01, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF };
    fwrite(unk, 1, 8, fo);
    seg_data_pos = ftell(fo);
    Bytes info, ib;
    ebml_elem(ib, 0x2AD7B1, be(1000000, 4));              // TimestampScale: 1 ms
    ebml_elem(ib, 0x4D80, str("libav1mi")); ebml_elem(ib, 0x5741, str("libav1mi"));
    ebml_id(ib, 0x4489); ebml_size(ib, 8);                 // Duration (float64 ms), patched at the end
    const size_t dur_off = ib.size();
    for (int i = 0; i < 8; i++) ib.push_back(0);
    ebml_elem(info, 0x1549A966, ib);
    const long info_pos = ftell(fo);
    fwrite(info.data(), 1, info.size(), fo);
    dur_pos = info_pos + (long)(info.size() - ib.size() + dur_off);
    // Tracks: one video track, CodecPrivate = AV1CodecConfigurationRecord (marker/version, profile/level, flags) + configOBUs
    Bytes tracks, te, vid, priv;
    priv.push_back(0x81); priv.push_back((uint8_t)((0 << 5) | 31));  // seq_profile 0, seq_level_idx 31 (as in the sequence header)
    priv.push_back((uint8_t)(((bit_depth > 8) << 6) | (1 << 3) | (1 << 2)));  // high_bitdepth, 4:2:0
    priv.push_back(0);
    priv.insert(priv.end(), seq_hdr_obu.begin(), seq_hdr_obu.end());
    ebml_elem(vid, 0xB0, be(w, 2)); ebml_elem(vid, 0xBA, be(h, 2));
    if (cp | tc | mc) {
      // Colour (Matroska): what the sequence header's colour description says, for players that read the container first
      Bytes col;
      ebml_elem(col, 0x55B1, be(mc ? mc : 2, 1));            // MatrixCoefficients
      ebml_elem(col, 0x55B2, be(bit_depth, 1));              // BitsPerChannel
      ebml_elem(col, 0x55B3, be(1, 1)); ebml_elem(col, 0x55B4, be(1, 1));   // ChromaSubsamplingHorz / Vert: 4:2:0
      ebml_elem(col, 0x55B9, be(full_range ? 2 : 1, 1));     // Range: 1 = broadcast, 2 = full
      ebml_elem(col, 0x55BA, be(tc ? tc : 2, 1));            // TransferCharacteristics
      ebml_elem(col, 0x55BB, be(cp ? cp : 2, 1));            // Primaries
      ebml_elem(vid, 0x55B0, col);
    }
    ebml_elem(te, 0xD7, be(1, 1)); ebml_elem(te, 0x73C5, be(1, 1)); ebml_elem(te, 0x83, be(1, 1)); ebml_elem(te, 0x9C, be(0, 1));
    ebml_elem(te, 0x86, str("V_AV1")); ebml_elem(te, 0x63A2, priv);
    ebml_elem(te, 0x23E383, be(1000000000ull * fps_d / fps_n, 4));  // DefaultDuration, ns
    ebml_elem(te, 0xE0, vid);
    Bytes tentry;
    ebml_elem(tentry, 0xAE, te);
    ebml_elem(tracks, 0x1654AE6B, tentry);
    fwrite(tracks.data(), 1, tracks.size(), fo);
    bytes = (uint64_t)ftell(fo);
  }
}

void Muxer::flush_cluster() {
  if (!cluster_open) return;
  Bytes c, body;
  ebml_elem(body, 0xE7, be(cluster_t0, 4));
  body.insert(body.end(), cluster.begin(), cluster.end());
  ebml_elem(c, 0x1F43B675, body);
  fwrite(c.data(), 1, c.size(), fo);
  bytes += c.size();
  cluster.clear();
  cluster_open = false;
}

void Muxer::write_frame(const uint8_t *tu, uint32_t size, bool key) {
  if (kind == IVF) {
    uint8_t fh[12];
    put_le(fh, size, 4); put_le(fh + 4, frames, 8);
    fwrite(fh, 1, 12, fo); fwrite(tu, 1, size, fo);
    bytes += 12 + size;
  } else if (kind == OBU) {
    fwrite(tu, 1, size, fo);
    bytes += size;
  } else {
    const uint64_t t = ts_ms(frames);
    if (key || !cluster_open || t - cluster_t0 > 30000) { flush_cluster(); cluster_open = true; cluster_t0 = t; }
    // SimpleBlock: track 1, int16 relative timestamp, flags (0x80 = key frame); the temporal delimiter is dropped
    const uint8_t *p = tu; uint32_t n = size;
    if (n >= 2 && p[0] == 0x12 && p[1] == 0x00) { p += 2; n -= 2; }
    ebml_id(cluster, 0xA3); ebml_size(cluster, 4 + (uint64_t)n);
    cluster.push_back(0x81);
    const int16_t rel = (int16_t)(t - cluster_t0);
    cluster.push_back((uint8_t)(rel >> 8)); cluster.push_back((uint8_t)rel);
    cluster.push_back(key ? 0x80 : 0x00);
    cluster.insert(cluster.end(), p, p + n);
  }
  frames++;
}

void Muxer::end() {
  if (kind == IVF) {
    if (fseek(fo, 24, SEEK_SET) == 0) { uint8_t cnt[4]; put_le(cnt, frames, 4); fwrite(cnt, 1, 4, fo); }
  } else if (kind == MKV) {
    flush_cluster();
    const long endpos = ftell(fo);
    Bytes sz;
    ebml_size(sz, (uint64_t)(endpos - seg_data_pos));
    if (fseek(fo, seg_size_pos, SEEK_SET) == 0) fwrite(sz.data(), 1, 8, fo);
    const double dur = (double)ts_ms(frames);
    uint64_t bits;
    memcpy(&bits, &dur, 8);
    Bytes d = be(bits, 8);
    if (fseek(fo, dur_pos, SEEK_SET) == 0) fwrite(d.data(), 1, 8, fo);
    fseek(fo, endpos, SEEK_SET);
  }
}

}  // namespace av1mi

extern "C" int av1mi_probe_y4m(const char *path, av1mi_clip_info *info) {
  if (!path || !info) return AV1MI_E_INVALID_ARG;
  av1mi::Y4m y;
  const int rc = av1mi::y4m_open(path, &y);
  if (rc) return rc;
  info->width = y.w; info->height = y.h; info->bit_depth = y.bd; info->fps_num = y.fps_n; info->fps_den = y.fps_d;
  info->color_range = y.color_range > 0 ? 1u : 0u;
  info->frames = y.total_frames;
  return AV1MI_OK;
}
