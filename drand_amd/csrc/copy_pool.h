// Host memcpy on a few pooled threads (pageable -> pinned runs at host memory
// bandwidth only when several cores copy), and the gather of scattered rows
// into one packed run on the same threads.  Host-only C++17, no HIP: capi.hip
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
  // Gather: row i (len[i] bytes at base + off[i], i < n) -> dst + (pos[i] -
  // pos[0]), the rows split across the pool in runs of equal byte share;
  // returns when every row is copied.  pos is ascending with pos[i + 1] >=
  // pos[i] + len[i] (the packed positions of the rows: a prefix sum of len),
  // so the runs write disjoint ranges of dst.
  void gather(void* dst, const uint8_t* base, const uint64_t* off, const uint32_t* len, const uint64_t* pos, size_t n) {
    if (!n) return;
    const size_t bytes = (size_t)(pos[n - 1] - pos[0]) + len[n - 1];
    const size_t parts = std::min(th_.size(), bytes / COPY_POOL_MIN_PART + (bytes % COPY_POOL_MIN_PART != 0));
    if (parts <= 1) {
      gather_rows((uint8_t*)dst, base, off, len, pos, pos[0], 0, n);
      return;
    }
    batch b;
    {
      std::lock_guard<std::mutex> lk(mu_);
      // run p ends at the first row whose packed position reaches share p + 1
      size_t lo = 0;
      for (size_t p = 0; p < parts && lo < n; ++p) {
        const uint64_t until = pos[0] + (uint64_t)(bytes / parts) * (p + 1);
        const size_t hi = p + 1 == parts ? n : (size_t)(std::lower_bound(pos + lo, pos + n, until) - pos);
        if (hi == lo) continue;
        task t{(uint8_t*)dst, base, hi - lo, &b};
        t.off = off + lo, t.len = len + lo, t.pos = pos + lo, t.pos0 = pos[0];
        q_.push_back(t);
        ++b.left;
        lo = hi;
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
    // a gather task (off != nullptr): n rows, d / s the bases of gather()
    const uint64_t* off = nullptr;
    const uint32_t* len = nullptr;
    const uint64_t* pos = nullptr;
    uint64_t pos0 = 0;
  };
  static void gather_rows(uint8_t* dst, const uint8_t* base, const uint64_t* off, const uint32_t* len,
                          const uint64_t* pos, uint64_t pos0, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i)
      if (len[i]) memcpy(dst + (pos[i] - pos0), base + off[i], len[i]);
  }
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
      if (t.off) gather_rows(t.d, t.s, t.off, t.len, t.pos, t.pos0, 0, t.n);
      else memcpy(t.d, t.s, t.n);
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
