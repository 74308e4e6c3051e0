// av1mi_file.cpp - av1mi_encode_file(): the in-process replacement of
//   pub fn run_av1an(params: &Av1anEncodeParams) -> Result<(), EncodeError>
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139), including the parts av1an does around the codec: splitting the clip into
// independent chunks (each starts with a key frame + sequence header; `--workers`/`--temp`, av1an.rs:100-104), running `workers` chunks
// in flight (one context each, round-robin over the visible GPUs) and concatenating chunk streams in order (SURVEY.md §8a rows a9, a20;
// §8e).  This file holds the job: its page-locked staging, the process-wide caches, the two chunk readers and the writer's rules.  The
// formats are av1mi_container.cpp's, the hand-over between reader, workers and writer is av1mi_pipeline.h's.  Output is written to a
// temporary name and renamed, so the caller's `exists && len > 0` validation (job_executor.rs:296-317) never sees a partial file.
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sched.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "av1mi_ctx.h"
#include "av1mi_container.h"
#include "av1mi_pipeline.h"

using namespace av1mi;

namespace {

// ---- host staging (BASELINE config 5 "per-GPU multi-stream overlap"; SURVEY.md §8e limiter "PCIe H2D of source frames") -------
// Chunks are read straight into PINNED host buffers (hipHostMalloc, portable across the job's GPUs) from a small pool: a
// context's upload of its next chunk is then a true asynchronous DMA at PCIe rate that runs beside the kernels of the other
// contexts on the same GPU (several contexts per GPU by default), instead of the runtime staging pageable memory through its
// own bounce buffer.  A slot goes back to the pool as soon as its chunk is encoded.
struct PinnedPool {
  struct Slot {
    uint8_t *p = nullptr; size_t cap = 0; bool busy = false, pinned = false;
    void free_mem() {
      if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
      p = nullptr; cap = 0; pinned = false;
    }
  };
  std::vector<Slot> slots;
  std::mutex mu;
  std::condition_variable cv;
  int device = 0;
  // Page-locked bytes this job may hold (AV1MI_PIN_BUDGET_MB, default 24 GiB - what the process-wide cache keeps anyway): slots
  // beyond it, and slots the runtime refuses to pin, are plain memory (the encode still works, their upload is staged by the runtime)
  size_t pin_budget = (size_t)24 << 30, pinned_bytes = 0;
  void init(int n, int dev);   // takes idle buffers from the process-wide cache
  void retire();               // gives them back
  Slot *acquire(size_t bytes) {
    std::unique_lock<std::mutex> lk(mu);
    Slot *s = nullptr;
    cv.wait(lk, [&] { for (auto &x : slots) if (!x.busy) { s = &x; return true; } return false; });
    s->busy = true;
    lk.unlock();
    if (s->cap < bytes) {
      release_mem(s);
      const size_t want = bytes + (bytes >> 3);
      bool may_pin;
      { std::lock_guard<std::mutex> lk2(mu); may_pin = pinned_bytes + want <= pin_budget; if (may_pin) pinned_bytes += want; }
      s->pinned = may_pin && hipSetDevice(device) == hipSuccess && hipHostMalloc((void **)&s->p, want, hipHostMallocPortable) == hipSuccess;
      if (!s->pinned) {
        if (may_pin) { (void)hipGetLastError(); std::lock_guard<std::mutex> lk2(mu); pinned_bytes -= want; }
        s->p = (uint8_t *)malloc(want);
      }
      s->cap = s->p ? want : 0;
    }
    return s;
  }
  void release(Slot *s) {
    { std::lock_guard<std::mutex> lk(mu); s->busy = false; }
    cv.notify_all();
  }
  void release_mem(Slot *s) {
    if (s->p && s->pinned) { std::lock_guard<std::mutex> lk2(mu); pinned_bytes -= s->cap < pinned_bytes ? s->cap : pinned_bytes; }
    s->free_mem();
  }
  ~PinnedPool() { retire(); }
};

// ---- process-wide caches ---------------------------------------------------------------------------------------------------
// The daemon is a long-lived process that encodes job after job (JobExecutor::execute, job_executor.rs:266-437): creating
// contexts (streams, several GB of HBM workspace each) and pinning host buffers per job cost more than a short clip's whole
// encode (measured: 4 contexts 50 ms, 6 pinned 373 MB slots ~60 ms to allocate and ~60 ms to free, against 18 ms of GPU work
// for 240 1080p frames).  Idle contexts and pinned slots are therefore kept between calls - "the per-GPU context owns its
// frame pool"  - bounded, and released by av1mi_release_caches().
struct GlobalCache {
  std::mutex mu;
  std::vector<std::pair<int, av1mi_ctx *>> ctxs;   // idle contexts (device, context)
  std::vector<PinnedPool::Slot> slots;             // idle host buffers
  size_t slot_bytes = 0;
};
GlobalCache &cache() { static GlobalCache *g = new GlobalCache(); return *g; }   // never destroyed: no HIP calls at process exit
const size_t kMaxCachedCtxPerDev = 8, kMaxCachedSlotBytes = (size_t)24 << 30;

void PinnedPool::init(int n, int dev) {
  slots.resize((size_t)n);
  device = dev;
  GlobalCache &g = cache();
  std::lock_guard<std::mutex> lk(g.mu);
  for (auto &s : slots) {
    if (g.slots.empty()) break;
    s = g.slots.back();
    s.busy = false;
    g.slot_bytes -= s.cap;
    if (s.pinned) pinned_bytes += s.cap;
    g.slots.pop_back();
  }
  if (const char *e = getenv("AV1MI_PIN_BUDGET_MB")) { const long mb = atol(e); if (mb >= 0) pin_budget = (size_t)mb << 20; }
}
void PinnedPool::retire() {
  GlobalCache &g = cache();
  for (auto &s : slots) {
    if (!s.p) continue;
    bool kept = false;
    {
      std::lock_guard<std::mutex> lk(g.mu);
      if (s.pinned && g.slot_bytes + s.cap <= kMaxCachedSlotBytes) { g.slots.push_back(s); g.slot_bytes += s.cap; kept = true; }
    }
    if (!kept) release_mem(&s);
  }
  slots.clear();
}

int take_ctx(int dev, av1mi_ctx **out) {
  {
    GlobalCache &g = cache();
    std::lock_guard<std::mutex> lk(g.mu);
    for (size_t i = 0; i < g.ctxs.size(); i++)
      if (g.ctxs[i].first == dev) { *out = g.ctxs[i].second; g.ctxs.erase(g.ctxs.begin() + (long)i); return AV1MI_OK; }
  }
  return av1mi_ctx_create(dev, out);
}
void give_ctx(int dev, av1mi_ctx *c) {
  if (!c) return;
  recycle_ctx(c);
  GlobalCache &g = cache();
  {
    std::lock_guard<std::mutex> lk(g.mu);
    size_t n = 0;
    for (auto &e : g.ctxs) n += e.first == dev;
    if (n < kMaxCachedCtxPerDev) { g.ctxs.emplace_back(dev, c); return; }
  }
  av1mi_ctx_destroy(c);
}

// One chunk on its way from the reader through a worker to the writer; owns its staging slot (until the upload is done) and its bitstream
struct Chunk {
  uint32_t index = 0, n_frames = 0, first_frame = 0;
  PinnedPool &pool;
  PinnedPool::Slot *slot;   // the chunk's frames: slot->p, pinned; p is null where no memory was to be had
  av1mi_buf out = { nullptr, 0 };
  std::vector<uint32_t> sizes;
  av1mi_report rep = {};
  std::vector<av1mi_plane_quality> quality;   // per [frame][plane], where the job asks for it (av1mi_encode_file_quality)
  int rc = 0;
  Chunk(PinnedPool &pl, size_t bytes) : pool(pl), slot(pl.acquire(bytes)) {}
  void release_slot() { if (slot) pool.release(slot); slot = nullptr; }
  ~Chunk() { release_slot(); av1mi_free(out.data); }
};
typedef std::unique_ptr<Chunk> ChunkPtr;
typedef OrderedPipeline<ChunkPtr> ChunkPipeline;

// phase times on stderr (AV1MI_TIMING; diagnostics)
struct Laps {
  const bool on = getenv("AV1MI_TIMING") != nullptr;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  void lap(const char *what) const { if (on) fprintf(stderr, "[av1mi_encode_file] %8.2f ms  %s\n", ms(), what); }
};

// What a job holds, and the one place it lets go of it.  On any failure the temporary file is unlinked; contexts go back to the cache -
// unless the encode failed, in which case release_device(true) has destroyed them: a context that saw a failure is not reused.
struct FileJob {
  Y4m clip;
  std::vector<std::pair<int, av1mi_ctx *>> ctxs;   // (device, context): the workers', then in scene mode the reader's
  std::string tmp;                                 // the temporary output's name while it exists
  FILE *fo = nullptr;
  PinnedPool pool;
  Laps laps;
  // the reader's and the writer's state
  int first_err = 0;
  uint32_t n_chunks = 0, frames_read = 0;

  int take(int dev) {
    av1mi_ctx *c = nullptr;
    const int rc = take_ctx(dev, &c);
    if (!rc) ctxs.emplace_back(dev, c);
    return rc;
  }
  void release_device(bool destroy) {
    for (auto &e : ctxs) { if (destroy) av1mi_ctx_destroy(e.second); else give_ctx(e.first, e.second); }
    ctxs.clear();
    pool.retire();
  }
  void fail(int rc) { if (!first_err) first_err = rc; }
  void submit(ChunkPipeline &pipe, ChunkPtr ck) {
    ck->index = n_chunks++;
    ck->first_frame = frames_read;
    frames_read += ck->n_frames;
    pipe.submit(std::move(ck));
  }
  ~FileJob() {
    release_device(false);
    if (fo) fclose(fo);
    if (!tmp.empty()) unlink(tmp.c_str());
  }
};

// reader: fixed-length chunks (every chunk starts with a key frame)
void read_fixed_chunks(FileJob &j, ChunkPipeline &pipe, uint32_t chunk_frames, int read_threads) {
  for (;;) {
    ChunkPtr ck(new Chunk(j.pool, (size_t)chunk_frames * j.clip.frame_bytes));
    if (!ck->slot->p) { j.fail(AV1MI_E_OOM); break; }
    int rerr = 0;
    ck->n_frames = y4m_read_frames(&j.clip, ck->slot->p, chunk_frames, read_threads, &rerr);
    if (rerr) j.fail(rerr);  // a malformed or truncated frame (AV1MI_E_FORMAT) or an I/O error
    if (ck->n_frames == 0) break;
    j.laps.lap("chunk read");
    j.submit(pipe, std::move(ck));
    if (j.first_err) break;
  }
}

// reader: chunks end at scene cuts (GPU luma-SAD pass per window of frames, include/av1mi.h: av1mi_scene_cuts)
void read_scene_chunks(FileJob &j, ChunkPipeline &pipe, av1mi_ctx *det_ctx, const av1mi_params &prm, int read_threads) {
  const uint32_t WIN = 32, MIN_SCENE = 12;
  const size_t frame_bytes = j.clip.frame_bytes;
  // a chunk's frames plus the window being examined stay under 4 GiB of pinned host memory
  const uint64_t cap = ((uint64_t)4 << 30) / frame_bytes;
  const uint32_t max_len = (uint32_t)(cap < MIN_SCENE + WIN ? MIN_SCENE : (cap - WIN > 240 ? 240 : cap - WIN));
  const size_t slot_bytes = (size_t)(max_len + WIN) * frame_bytes;
  std::vector<uint8_t> prev(frame_bytes);
  std::vector<uint8_t> cuts(WIN);
  bool has_prev = false;
  av1mi_scene_state st = {};
  // Windows are read straight behind the current chunk's frames in its pinned slot and examined there; only where a chunk
  // ends inside a window do the frames after the cut move to the next chunk's slot.
  ChunkPtr cur(new Chunk(j.pool, slot_bytes));
  bool oom = !cur->slot->p;
  while (!oom && !j.first_err) {
    uint8_t *win = cur->slot->p + (size_t)cur->n_frames * frame_bytes;
    int rerr = 0;
    const uint32_t nw = y4m_read_frames(&j.clip, win, WIN, read_threads, &rerr);
    if (rerr) j.fail(rerr);  // a malformed or truncated frame (AV1MI_E_FORMAT) or an I/O error
    if (nw == 0) break;
    const int src = av1mi_scene_cuts(det_ctx, &prm, win, nw, 0, has_prev ? prev.data() : nullptr, &st, MIN_SCENE, nullptr, cuts.data());
    if (src) { j.fail(src); break; }
    memcpy(prev.data(), win + (size_t)(nw - 1) * frame_bytes, frame_bytes);
    has_prev = true;
    for (uint32_t t = 0; t < nw; t++) {
      if ((cuts[t] && cur->n_frames > 0) || cur->n_frames == max_len) {
        // frame t starts the next chunk: it and the rest of the window move to a slot of their own
        ChunkPtr nx(new Chunk(j.pool, slot_bytes));
        if (!nx->slot->p) { oom = true; break; }
        memcpy(nx->slot->p, cur->slot->p + (size_t)cur->n_frames * frame_bytes, (size_t)(nw - t) * frame_bytes);
        j.submit(pipe, std::move(cur));
        cur = std::move(nx);
      }
      cur->n_frames++;   // (the frame already sits in place: the window was read behind the chunk's frames)
    }
  }
  if (oom) j.fail(AV1MI_E_OOM);
  if (cur->n_frames > 0 && !j.first_err) j.submit(pipe, std::move(cur));
}

// ... and the planes' quality sums, where the job has them: the windows of a long clip outgrow 32 bits, `reserved` carries the high half
void add_report(av1mi_report &tot, av1mi_plane_quality *sum, const Chunk &ck) {
  const av1mi_report &r = ck.rep;
  for (size_t i = 0; sum && i < ck.quality.size(); i++) {
    av1mi_plane_quality &s = sum[i % 3];
    const uint64_t n = ((uint64_t)s.reserved << 32 | s.windows) + ck.quality[i].windows;
    s.sse += ck.quality[i].sse; s.ssim_sum += ck.quality[i].ssim_sum;
    s.windows = (uint32_t)n; s.reserved = (uint32_t)(n >> 32);
  }
  tot.frames += ck.n_frames; tot.bytes += r.bytes; tot.n_symbols += r.n_symbols;
  tot.gpus_used |= r.gpus_used;
  for (int p = 0; p < 3; p++) tot.sse[p] += r.sse[p];
  tot.ms_recon += r.ms_recon; tot.ms_cdef += r.ms_cdef; tot.ms_entropy += r.ms_entropy;
  tot.ms_pack += r.ms_pack; tot.ms_h2d += r.ms_h2d; tot.ms_d2h += r.ms_d2h; tot.ms_total += r.ms_total;
}

void finish_psnr(av1mi_report &tot, const Y4m &clip) {
  const double mx = (double)((1 << clip.bd) - 1);
  for (int p = 0; p < 3; p++) {
    const double npx = (double)tot.frames * clip.w * clip.h / (p ? 4 : 1);
    tot.psnr[p] = tot.sse[p] > 0 ? 10.0 * log10(mx * mx * npx / tot.sse[p]) : 99.0;
  }
}

// the reader threads: by the cores this process may use, not the host's
int plan_read_threads() {
  int hc = 0;
  { cpu_set_t cs; if (sched_getaffinity(0, sizeof(cs), &cs) == 0) hc = CPU_COUNT(&cs); }
  if (hc <= 0) hc = (int)std::thread::hardware_concurrency();
  int read_threads = hc >= 16 ? 12 : (hc >= 8 ? 6 : (hc >= 4 ? 3 : 1));
  if (const char *e = getenv("AV1MI_READ_THREADS")) { const int k = atoi(e); if (k > 0 && k <= 64) read_threads = k; }
  return read_threads;
}

}  // namespace

// ---- chunk -> GPU placement: the two rules everything multi-GPU in this build goes through ----------------
extern "C" uint32_t av1mi_chunk_owner(uint32_t chunk_index, uint32_t n_owners) { return n_owners ? chunk_index % n_owners : 0u; }

extern "C" int av1mi_plan_workers(uint32_t workers, int32_t gpu_mask, int n_devices, int32_t *device_of_worker, uint32_t cap) {
  if (n_devices <= 0) return 0;
  int devs[64], nd = 0;
  for (int d = 0; d < n_devices && d < 32 && nd < 64; d++) if (gpu_mask <= 0 || ((gpu_mask >> d) & 1)) devs[nd++] = d;
  if (nd == 0) return 0;
  // default: AV1MI_DEFAULT_WORKERS_PER_GPU chunks in flight per allowed GPU - a chunk's P-frame chain is latency bound, chains of
  // different chunks overlap (the reference runs `--workers 8` on one host, concurrency.rs:67-73)
  uint32_t w = workers ? workers : (uint32_t)nd * AV1MI_DEFAULT_WORKERS_PER_GPU;
  if (w > 64) w = 64;
  for (uint32_t i = 0; i < w && i < cap; i++) if (device_of_worker) device_of_worker[i] = devs[av1mi_chunk_owner(i, (uint32_t)nd)];
  return (int)w;
}

extern "C" void av1mi_release_caches(void) {
  GlobalCache &g = cache();
  std::vector<std::pair<int, av1mi_ctx *>> cs;
  std::vector<PinnedPool::Slot> ss;
  {
    std::lock_guard<std::mutex> lk(g.mu);
    cs.swap(g.ctxs);
    ss.swap(g.slots);
    g.slot_bytes = 0;
  }
  for (auto &e : cs) av1mi_ctx_destroy(e.second);
  for (auto &s : ss) s.free_mem();
  release_streams();   // the stream sets destroyed contexts left in av1mi_ctx.cpp's pool
  release_buffers();   // and the page-locked bitstream blocks av1mi_free() put back
}

extern "C" int av1mi_encode_file(const av1mi_job *job, av1mi_progress_cb cb, void *user, av1mi_report *total) {
  return av1mi_encode_file_quality(job, cb, user, total, nullptr);
}

// sum: null, or the job's quality sums - its workers' contexts then run the quality pass on every chunk (give_ctx switches it off again)
extern "C" int av1mi_encode_file_quality(const av1mi_job *job, av1mi_progress_cb cb, void *user, av1mi_report *total, av1mi_plane_quality sum[3]) {
  if (!job || !job->input_path || !job->output_path) return AV1MI_E_INVALID_ARG;
  FileJob j;   // every return below releases what the job holds by then
  const Laps &laps = j.laps;
  const Y4m &y = j.clip;
  int rc = y4m_open(job->input_path, &j.clip);
  if (rc) return rc;
  av1mi_params prm = job->params;
  prm.width = y.w; prm.height = y.h; prm.bit_depth = y.bd;
  if (y.color_range >= 0) prm.color_range = (uint32_t)y.color_range;  // the clip's own tag wins over the job's default
  const bool scene_mode = job->chunk_frames == 0;
  const uint32_t chunk_frames = job->chunk_frames ? job->chunk_frames : 60;
  // contexts: `workers` chunks in flight, spread round-robin over the allowed GPUs
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AV1MI_E_NO_DEVICE;
  int32_t dev_of[64];
  const int planned = av1mi_plan_workers(job->workers, job->gpu_mask, ndev, dev_of, 64);
  if (planned <= 0) return AV1MI_E_NO_DEVICE;
  const uint32_t workers = (uint32_t)planned;
  for (uint32_t i = 0; i < workers; i++)
    if ((rc = j.take(dev_of[i]))) return rc;
  if (sum) for (auto &e : j.ctxs) (void)av1mi_ctx_set_quality(e.second, 1);
  laps.lap("contexts created");
  if (scene_mode && (rc = j.take(dev_of[0]))) return rc;   // the reader thread's own context for the scene-cut pass; gets no worker thread
  av1mi_ctx *det_ctx = scene_mode ? j.ctxs.back().second : nullptr;
  j.tmp = std::string(job->output_path) + ".tmp." + std::to_string((long)getpid());
  j.fo = fopen(j.tmp.c_str(), "wb");
  if (!j.fo) { const int e = -errno; j.tmp.clear(); return e; }
  Muxer mux(j.fo, job->output_path, y, prm);
  {
    uint8_t sh[64]; size_t shn = sizeof(sh);
    rc = av1mi_write_headers(&prm, sh, &shn, nullptr, nullptr);
    if (rc) return rc;
    mux.begin(std::vector<uint8_t>(sh, sh + shn));
  }

  // pinned staging: one slot being filled by the reader, one waiting, one per worker being uploaded / encoded
  j.pool.init((int)workers + 2, dev_of[0]);
  expect_blocks(2 * workers + 2);   // finished chunks waiting for the writer keep their page-locked output blocks
  const int read_threads = plan_read_threads();

  const auto t0 = std::chrono::steady_clock::now();
  uint32_t frames_done = 0;
  const uint32_t keyint = prm.keyint ? prm.keyint : 1;
  av1mi_report tot = {};
  av1mi_plane_quality qtot[3] = {};
  auto encode = [&](ChunkPtr &ck, unsigned worker) {
    ck->sizes.resize(ck->n_frames);
    av1mi_params cp = prm;
    cp.first_frame = prm.first_frame + ck->first_frame;
    ck->rc = av1mi_encode_chunk(j.ctxs[worker].second, &cp, ck->slot->p, ck->n_frames, 0, &ck->out, ck->sizes.data(), nullptr, &ck->rep);
    if (sum && !ck->rc) {
      ck->quality.resize((size_t)ck->n_frames * 3);
      ck->rc = av1mi_quality_result(j.ctxs[worker].second, ck->n_frames, ck->quality.data());
    }
    if (laps.on) fprintf(stderr, "[av1mi_encode_file] %8.2f ms  chunk %u encoded (h2d %.2f total %.2f ms on the device)\n", laps.ms(), ck->index, ck->rep.ms_h2d, ck->rep.ms_total);
    ck->release_slot();   // (av1mi_encode_chunk returns after its upload has completed)
  };
  // the writer: after the first failed chunk nothing more is written (every chunk is still taken, freed and counted by the pipeline)
  auto write = [&](ChunkPtr &ck) {
    if (ck->rc) j.fail(ck->rc);
    if (j.first_err) return;
    size_t off = 0;
    for (uint32_t f = 0; f < ck->n_frames; f++) {
      mux.write_frame(ck->out.data + off, ck->sizes[f], f % keyint == 0);
      off += ck->sizes[f];
    }
    frames_done += ck->n_frames;
    add_report(tot, sum ? qtot : nullptr, *ck);
    if (cb) {
      const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      // total: the clip's length when the input is a regular file, else the frames read so far
      const uint32_t tot_frames = y.total_frames >= j.frames_read ? (uint32_t)y.total_frames : j.frames_read;
      cb(user, frames_done, tot_frames, sec > 0 ? frames_done / sec : 0.0, mux.bytes);
    }
  };
  {
    ChunkPipeline pipe(workers, encode, write);
    if (scene_mode) read_scene_chunks(j, pipe, det_ctx, prm, read_threads);
    else read_fixed_chunks(j, pipe, chunk_frames, read_threads);
    laps.lap("input consumed");
    pipe.finish();
    laps.lap("all chunks written");
  }
  j.release_device(j.first_err != 0);
  laps.lap("contexts and host buffers back in the cache");
  // patch frame count, finish atomically
  mux.end();
  const int io_err = (fflush(j.fo) != 0 || ferror(j.fo)) ? -EIO : 0;
  fclose(j.fo);
  j.fo = nullptr;
  if (!j.first_err && !io_err && frames_done == 0) j.first_err = AV1MI_E_FORMAT;
  if (j.first_err || io_err) return j.first_err ? j.first_err : io_err;
  if (rename(j.tmp.c_str(), job->output_path) != 0) return -errno;
  j.tmp.clear();
  if (total) {
    finish_psnr(tot, y);
    tot.chunks = j.n_chunks;
    *total = tot;
  }
  if (sum) memcpy(sum, qtot, sizeof(qtot));
  return AV1MI_OK;
}
