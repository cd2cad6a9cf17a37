// Host memcpy on a few pooled threads (pageable -> pinned runs at host memory
// bandwidth only when several cores copy).  Host-only C++17, no HIP: capi.hip
// fills the staging ring's pinned slots through it, and
// tests/copy_pool_check.cpp builds it alone under the host sanitizers.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

// smallest part worth a thread of its own
constexpr size_t COPY_POOL_MIN_PART = 1 << 20;

// How a copy of `bytes` is split over at most `threads` threads: `parts`
// parts of `per` bytes, part p = [min(bytes, p * per), min(bytes, (p + 1) * per)).
// per is a multiple of 64 (every part starts on a cache line of the copy) and
// parts * per >= bytes: the parts cover the copy exactly; trailing parts may
// be empty.  (per was round_up_64(floor(bytes / parts)) once: where that
// quotient was a multiple of 64 already and bytes % parts != 0, the last
// bytes % parts bytes were never copied.)
struct copy_split {
  size_t parts, per;
  size_t off(size_t bytes, size_t p) const { return std::min(bytes, p * per); }
  size_t len(size_t bytes, size_t p) const { return std::min(bytes - off(bytes, p), per); }
};

inline copy_split copy_pool_split(size_t bytes, size_t threads, size_t min_part = COPY_POOL_MIN_PART) {
  const size_t parts = std::min(threads, bytes / min_part + (bytes % min_part != 0));
  if (parts <= 1) return copy_split{parts, bytes};
  const size_t per = (bytes / parts + (bytes % parts != 0) + 63) & ~(size_t)63;
  return copy_split{parts, per};
}

class copy_pool {
 public:
  explicit copy_pool(int threads) {
    for (int i = 0; i < threads; ++i) th_.emplace_back([this] { work(); });
  }
  ~copy_pool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // dst <- src (bytes), split across the pool; returns when every part is done
  void copy(void* dst, const void* src, size_t bytes) {
    const copy_split sp = copy_pool_split(bytes, th_.size());
    if (sp.parts <= 1) {
      if (bytes) memcpy(dst, src, bytes);
      return;
    }
    batch b;
    b.left = sp.parts;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (size_t p = 0; p < sp.parts; ++p) {
        const size_t off = sp.off(bytes, p);
        q_.push_back(task{(uint8_t*)dst + off, (const uint8_t*)src + off, sp.len(bytes, p), &b});
      }
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(b.mu);
    b.cv.wait(lk, [&] { return b.left == 0; });
  }

 private:
  struct batch {
    std::mutex mu;
    std::condition_variable cv;
    size_t left = 0;
  };
  struct task {
    uint8_t* d;
    const uint8_t* s;
    size_t n;
    batch* b;
  };
  void work() {
    for (;;) {
      task t;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        t = q_.front();
        q_.pop_front();
      }
      memcpy(t.d, t.s, t.n);
      std::lock_guard<std::mutex> lk(t.b->mu);
      if (--t.b->left == 0) t.b->cv.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<task> q_;
  bool stop_ = false;
};
