// av1mi_pipeline.h - the ordered, bounded hand-over of av1mi_encode_file: one thread submits items, `workers` threads of the pipeline's own
// work on them in any order, and the submitting thread writes them in submission order.  Standard library only, no GPU
// (tests/host/pipeline_host.cpp runs it under ThreadSanitizer).  What a failed item means is the caller's business: `write` sees every
// item, in order, and decides.
#ifndef AV1MI_PIPELINE_H
#define AV1MI_PIPELINE_H
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace av1mi {

template <class Item>   // movable, with an empty default state (a smart pointer); the pipeline owns an item from submit() until write() has returned, then destroys it
class OrderedPipeline {
 public:
  typedef std::function<void(Item &, unsigned worker_index)> Work;   // on one of the pipeline's threads
  typedef std::function<void(Item &)> Write;                         // on the submitting thread, in submission order

  OrderedPipeline(unsigned workers, Work work, Write write) : workers_(workers), work_(std::move(work)), write_(std::move(write)) {
    for (unsigned i = 0; i < workers; i++) threads_.emplace_back([this, i] { run(i); });
  }
  ~OrderedPipeline() { finish(); }
  OrderedPipeline(const OrderedPipeline &) = delete;
  OrderedPipeline &operator=(const OrderedPipeline &) = delete;

  void submit(Item item) {
    // Bound the items held in memory: at most 2 * workers submitted but not yet written.  Finished items are written
    // by THIS thread, so while waiting it must keep draining - waiting only for "fewer outstanding" would deadlock
    // once every outstanding item is finished and parked in `done_`.
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return submitted_ - written_ < 2 * (uint64_t)workers_ || done_.count(written_); });
        if (submitted_ - written_ < 2 * (uint64_t)workers_) {
          queue_.emplace_back(submitted_++, std::move(item));
          break;
        }
      }
      drain(false);
    }
    cv_work_.notify_one();
    drain(false);
  }

  // no more input: writes the rest in order and joins the workers
  void finish() {
    { std::lock_guard<std::mutex> lk(mu_); eof_ = true; }
    cv_work_.notify_all();
    drain(true);
    for (auto &t : threads_) t.join();
    threads_.clear();
  }

 private:
  void run(unsigned index) {
    for (;;) {
      std::pair<uint64_t, Item> e;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_work_.wait(lk, [&] { return !queue_.empty() || eof_; });
        if (queue_.empty()) return;
        e = std::move(queue_.front());
        queue_.pop_front();
      }
      work_(e.second, index);
      { std::lock_guard<std::mutex> lk(mu_); done_.emplace(e.first, std::move(e.second)); }
      cv_done_.notify_all();
    }
  }
  // writes the finished items that are next in order; all: waits for every submitted item
  void drain(bool all) {
    for (;;) {
      Item item;
      {
        std::unique_lock<std::mutex> lk(mu_);
        if (all) cv_done_.wait(lk, [&] { return written_ >= submitted_ || done_.count(written_); });
        auto it = done_.find(written_);
        if (written_ >= submitted_ || it == done_.end()) return;
        item = std::move(it->second);
        done_.erase(it);
      }
      write_(item);
      written_++;
    }
  }

  const unsigned workers_;
  Work work_;
  Write write_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  std::deque<std::pair<uint64_t, Item>> queue_;   // submitted, waiting for a worker
  std::map<uint64_t, Item> done_;                 // worked on, waiting for their turn to be written
  uint64_t submitted_ = 0, written_ = 0;          // (both move on the submitting thread alone)
  bool eof_ = false;
  std::vector<std::thread> threads_;
};

}  // namespace av1mi

#endif
