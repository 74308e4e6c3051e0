// av1mi_encode_file's hand-over between reader, workers and writer (av1-base_amd/csrc/av1mi_pipeline.h) as a stand-alone program, run plain,
// under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer (tests/test_pipeline_host.py):
//   pipeline_host <workers> <items> <fail_at, or -1> [<workers> <items> <fail_at> ...]      one pipeline and one line of output per triple
// The items' work sleeps, longer for earlier items, so later items finish first; item `fail_at` fails with code 100 + fail_at, and the
// caller keeps av1mi_file.cpp's rule: the first failure is remembered, nothing is written from then on, and the reader stops submitting
// once it sees the failure.  Prints what happened on one line; the items are heap objects, so one that is lost is a leak.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

#include "../../av1-base_amd/csrc/av1mi_pipeline.h"

static std::atomic<int> g_made(0), g_gone(0);

struct Item {
  int id, rc = 0;
  bool worked = false;
  explicit Item(int i) : id(i) { g_made++; }
  ~Item() { g_gone++; }
};
typedef std::unique_ptr<Item> ItemPtr;

static void run(int workers, int items, int fail_at) {
  g_made = 0;
  g_gone = 0;
  const std::thread::id me = std::this_thread::get_id();
  std::atomic<int> n_written(0), max_out(0), bad_worker(0);
  auto saw = [&](int accepted) {   // `accepted` items are known to be in the pipeline: those minus the written ones are outstanding
    const int out = accepted - n_written.load();
    for (int cur = max_out.load(); out > cur && !max_out.compare_exchange_weak(cur, out);) { }
  };
  std::vector<int> order;
  int first_err = 0, wrong_thread = 0, unworked = 0, submitted = 0;
  {
    av1mi::OrderedPipeline<ItemPtr> pipe(
        (unsigned)workers,
        [&](ItemPtr &it, unsigned w) {
          saw(it->id + 1);
          if (w >= (unsigned)workers) bad_worker++;
          std::this_thread::sleep_for(std::chrono::microseconds(200 + 20 * (items - 1 - it->id)));   // 40 items: 23.6 ms in all, 14 such runs well under a second
          it->worked = true;
          if (it->id == fail_at) it->rc = 100 + fail_at;
        },
        [&](ItemPtr &it) {
          if (std::this_thread::get_id() != me) wrong_thread++;
          if (!it->worked) unworked++;
          n_written++;
          if (it->rc && !first_err) first_err = it->rc;
          if (first_err) return;
          order.push_back(it->id);
        });
    for (int i = 0; i < items; i++) {
      pipe.submit(ItemPtr(new Item(i)));
      submitted = i + 1;
      saw(submitted);
      if (first_err) break;
    }
    pipe.finish();
  }
  printf("workers=%d submitted=%d seen=%d err=%d max_outstanding=%d wrong_thread=%d unworked=%d bad_worker=%d made=%d gone=%d written=", workers, submitted,
         n_written.load(), first_err, max_out.load(), wrong_thread, unworked, bad_worker.load(), g_made.load(), g_gone.load());
  for (int id : order) printf("%d,", id);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: pipeline_host <workers> <items> <fail_at> ...\n"); return 2; }
  for (int a = 1; a + 2 < argc; a += 3) run(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]));
  return 0;
}
