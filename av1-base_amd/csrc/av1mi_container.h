// av1mi_container.h - the clip in and the file out of av1mi_encode_file: the Y4M reader and the three output containers.  Nothing here
// touches the GPU: av1mi_container.cpp includes no HIP header, the plain host compiler builds it (tests/host/container_host.cpp).
#ifndef AV1MI_CONTAINER_H
#define AV1MI_CONTAINER_H
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/av1mi.h"

namespace av1mi {

// An open Y4M clip; owns its FILE.
struct Y4m {
  FILE *f = nullptr;
  uint32_t w = 0, h = 0, bd = 8, fps_n = 30, fps_d = 1;   // (y4m_open leaves no rate of 0: a missing or zero rate is 30:1)
  int color_range = -1;       // XCOLORRANGE tag: 0 LIMITED, 1 FULL, -1 absent
  size_t frame_bytes = 0;
  uint64_t total_frames = 0;  // from the file size (plain "FRAME\n" markers); 0 = unknown (pipe)
  long data_off = 0;          // file offset of the first FRAME marker
  uint64_t next_frame = 0;    // frames handed out so far (regular files: position of the next frame)
  bool regular = false;       // seekable regular file: frames can be read in parallel with pread
  Y4m() = default;
  Y4m(const Y4m &) = delete;
  Y4m &operator=(const Y4m &) = delete;
  ~Y4m() { if (f) fclose(f); }
};

int y4m_open(const char *path, Y4m *y);
// returns 1 frame read, 0 clean EOF, <0 error
int y4m_read_frame(Y4m *y, uint8_t *dst);
// Reads the next `count` frames into dst (tight I420, frame after frame), regular files with up to `threads` parallel readers.  Returns
// the number of whole frames read (short at end of file); *err receives a format / IO error.
uint32_t y4m_read_frames(Y4m *y, uint8_t *dst, uint32_t count, int threads, int *err);

void put_le(uint8_t *p, uint64_t v, int n);

// The output file.  The container is chosen by the extension of the output path: .mkv/.webm -> Matroska (EBML header, Segment{Info,
// Tracks{V_AV1 + av1C CodecPrivate}, Clusters of SimpleBlocks}), .obu -> bare Section-5 OBU stream, anything else -> IVF.  Video only: the
// Y4M input has no audio to pass through.
struct Muxer {
  enum Kind { IVF, MKV, OBU };
  // what the file says of the clip: its size, rate and bit depth, and the job's colour description (av1mi_params; 0 = none)
  Muxer(FILE *out, const char *output_path, const Y4m &clip, const av1mi_params &prm);
  void begin(const std::vector<uint8_t> &seq_hdr_obu);
  // one temporal unit (TD + [sequence header] + frame); `key`: starts a new cluster in Matroska
  void write_frame(const uint8_t *tu, uint32_t size, bool key);
  void end();   // patches the frame count (IVF), the segment size and the duration (Matroska)

  FILE *fo;
  Kind kind;
  bool webm;
  uint32_t w, h, fps_n, fps_d, bit_depth;
  uint32_t cp, tc, mc;
  bool full_range;
  uint64_t frames = 0, bytes = 0;

 private:
  uint64_t ts_ms(uint64_t frame) const { return frame * 1000ull * fps_d / fps_n; }
  void flush_cluster();
  long seg_size_pos = 0, seg_data_pos = 0, dur_pos = 0;
  std::vector<uint8_t> cluster;     // SimpleBlocks of the open cluster
  uint64_t cluster_t0 = 0;          // its timestamp, ms
  bool cluster_open = false;
};

}  // namespace av1mi

#endif
