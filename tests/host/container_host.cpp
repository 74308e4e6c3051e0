// The file formats of av1mi_encode_file (av1-base_amd/csrc/av1mi_container.cpp) as a stand-alone program for the plain host compiler, with
// and without sanitizers (tests/test_container_host.py).  It reads commands, one per line, from <dir>/commands.txt, works in <dir>, and
// prints one line per command with what the code under test returned; frames read and files muxed are written to <dir> for the Python
// side to compare.
//   probe <clip>                                      av1mi_probe_y4m
//   read <clip> <window> <threads> <out>              y4m_read_frames until it returns 0; the frames go to <out>
//   fifo <clip> <window> <out>                        the same through a FIFO that a second thread feeds with <clip>'s bytes
//   mux <units> <out> <seq hex> <w> <h> <fps_n> <fps_d> <bit depth> <cp> <tc> <mc> <full range>
//       <units>: per temporal unit one byte key flag, four bytes size (little endian), the bytes
#include <fcntl.h>
#include <signal.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../av1-base_amd/csrc/av1mi_container.h"

using namespace av1mi;

static std::vector<uint8_t> slurp(const std::string &path) {
  std::vector<uint8_t> v;
  if (FILE *f = fopen(path.c_str(), "rb")) {
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
  }
  return v;
}

static void probe(const std::string &clip) {
  av1mi_clip_info ci;
  memset(&ci, 0xEE, sizeof(ci));
  const int rc = av1mi_probe_y4m(clip.c_str(), &ci);
  printf("probe rc=%d", rc);
  if (!rc) printf(" w=%u h=%u bd=%u fps=%u:%u cr=%u frames=%llu", ci.width, ci.height, ci.bit_depth, ci.fps_num, ci.fps_den, ci.color_range, (unsigned long long)ci.frames);
  printf("\n");
}

// every window's count, the last error, and what the clip knows of itself
static void read_all(const std::string &clip, uint32_t window, int threads, const std::string &out) {
  Y4m y;
  const int rc = y4m_open(clip.c_str(), &y);
  printf("read open=%d", rc);
  if (rc) { printf("\n"); return; }
  printf(" regular=%d total=%llu counts=", y.regular ? 1 : 0, (unsigned long long)y.total_frames);
  FILE *fo = fopen(out.c_str(), "wb");
  std::vector<uint8_t> buf((size_t)window * y.frame_bytes);
  int err = 0;
  for (;;) {
    const uint32_t n = y4m_read_frames(&y, buf.data(), window, threads, &err);
    printf("%u,", n);
    if (fo) fwrite(buf.data(), 1, (size_t)n * y.frame_bytes, fo);
    if (n == 0 || err) break;
  }
  if (fo) fclose(fo);
  printf(" err=%d\n", err);
}

static void mux(std::istringstream &args) {
  std::string units_path, out, seq_hex;
  Y4m clip;
  av1mi_params prm;
  memset(&prm, 0, sizeof(prm));
  args >> units_path >> out >> seq_hex >> clip.w >> clip.h >> clip.fps_n >> clip.fps_d >> clip.bd >> prm.color_primaries >> prm.transfer_characteristics >>
      prm.matrix_coefficients >> prm.color_range;
  std::vector<uint8_t> seq;
  for (size_t i = 0; i + 1 < seq_hex.size(); i += 2) seq.push_back((uint8_t)strtoul(seq_hex.substr(i, 2).c_str(), nullptr, 16));
  const std::vector<uint8_t> units = slurp(units_path);
  FILE *fo = fopen(out.c_str(), "wb");
  if (!fo) { printf("mux open failed\n"); return; }
  Muxer m(fo, out.c_str(), clip, prm);
  m.begin(seq);
  for (size_t at = 0; at + 5 <= units.size();) {
    const bool key = units[at] != 0;
    const uint32_t size = units[at + 1] | units[at + 2] << 8 | units[at + 3] << 16 | (uint32_t)units[at + 4] << 24;
    m.write_frame(units.data() + at + 5, size, key);
    at += 5 + size;
  }
  m.end();
  const int bad = fflush(fo) != 0 || ferror(fo);
  fclose(fo);
  printf("mux kind=%d frames=%llu bytes=%llu io=%d\n", (int)m.kind, (unsigned long long)m.frames, (unsigned long long)m.bytes, bad);
}

int main(int argc, char **argv) {
  if (argc < 2 || chdir(argv[1]) != 0) { fprintf(stderr, "usage: container_host <directory with commands.txt>\n"); return 2; }
  signal(SIGPIPE, SIG_IGN);   // a reader that gives up on the FIFO early must not kill the program
  FILE *f = fopen("commands.txt", "r");
  if (!f) { fprintf(stderr, "no commands.txt\n"); return 2; }
  char line[4096];
  while (fgets(line, sizeof(line), f)) {
    std::istringstream args(line);
    std::string cmd, clip, out;
    uint32_t window = 0;
    int threads = 1;
    args >> cmd;
    if (cmd == "probe") {
      args >> clip;
      probe(clip);
    } else if (cmd == "read") {
      args >> clip >> window >> threads >> out;
      read_all(clip, window, threads, out);
    } else if (cmd == "fifo") {
      args >> clip >> window >> out;
      const std::string fifo = out + ".fifo";
      unlink(fifo.c_str());
      if (mkfifo(fifo.c_str(), 0600) != 0) { printf("fifo mkfifo failed\n"); continue; }
      std::thread feeder([&] {
        const std::vector<uint8_t> bytes = slurp(clip);
        const int fd = open(fifo.c_str(), O_WRONLY);
        for (size_t at = 0; fd >= 0 && at < bytes.size();) {
          const ssize_t n = write(fd, bytes.data() + at, bytes.size() - at < 1000 ? bytes.size() - at : 1000);
          if (n <= 0) break;
          at += (size_t)n;
        }
        if (fd >= 0) close(fd);
      });
      read_all(fifo, window, 4, out);
      feeder.join();
      unlink(fifo.c_str());
    } else if (cmd == "mux") {
      mux(args);
    } else if (!cmd.empty()) {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  fclose(f);
  return 0;
}
