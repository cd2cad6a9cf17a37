// Host check of drand_amd/csrc/copy_pool.h, the pool that copies a caller's
// host records into the staging ring's pinned slots (capi.hip
// ring_copy_locked).  Built by tests/test_copy_pool.py under ASan + UBSan
// (all parts) and under TSan (the concurrent part).
//
//   copy_pool_check split       every bytes in [1, 16 MiB + 64], 8 threads: the
//                               parts are in order, disjoint, start on 64-byte
//                               boundaries, stay inside the copy and cover it
//   copy_pool_check copy        byte-exact copies through a pool of 8 threads
//                               at the sizes where a split can lose its tail,
//                               aligned and misaligned, canaries around dst
//   copy_pool_check concurrent  8 callers x 50 copies through one pool at once
//   copy_pool_check             all three
//
// Prints one line per failing size (at most 20 per part) and a summary line;
// exit status 0 only when nothing failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "copy_pool.h"

namespace {

constexpr size_t MiB = 1 << 20;
constexpr size_t SLOT = 16 * MiB;  // capi.hip STAGE_SLOT_BYTES: the largest copy the ring makes
constexpr size_t THREADS = 8;      // capi.hip STAGE_COPY_THREADS
constexpr size_t CANARY = 256;
constexpr size_t MAX_OFF = 64;
constexpr int REPORT = 20;

// ---------------------------------------------------------------- split properties
size_t check_split(size_t* failures) {
  size_t swept = 0;
  int shown = 0;
  for (size_t bytes = 1; bytes <= SLOT + 64; ++bytes, ++swept) {
    const copy_split s = copy_pool_split(bytes, THREADS);
    const size_t want = std::min(THREADS, (bytes + MiB - 1) / MiB);
    const char* why = nullptr;
    size_t pos = 0;
    if (s.parts != want) why = "part count";
    for (size_t p = 0; p < s.parts && !why; ++p) {
      const size_t off = s.off(bytes, p), len = s.len(bytes, p);
      if (off != pos) why = off < pos ? "parts overlap" : "gap between parts";
      else if (len && off % 64) why = "part start not 64-byte aligned";
      else if (off > bytes || len > bytes - off) why = "part extends past the copy";
      pos = off + len;
    }
    if (!why && pos != bytes) why = "tail not covered";
    if (why) {
      ++*failures;
      if (shown++ < REPORT)
        printf("split FAIL bytes=%zu parts=%zu per=%zu covered=%zu: %s\n", bytes, s.parts, s.per, pos, why);
    }
  }
  return swept;
}

// ---------------------------------------------------------------- byte-exact copies
uint8_t pattern(size_t i) { return (uint8_t)(i * 131 + (i >> 8) * 31 + (i >> 16) * 7 + 1); }

// The source of every copy: a position-dependent pattern, and its complement
// (what a destination holds before a copy, so a byte that is not copied
// differs from the source whatever its position).  Read-only once built.
struct patterns {
  std::vector<uint8_t> src, fill;
  patterns() : src(SLOT + MAX_OFF), fill(SLOT + MAX_OFF) {
    for (size_t i = 0; i < src.size(); ++i) {
      src[i] = pattern(i);
      fill[i] = (uint8_t)~src[i];
    }
  }
};

// One caller's destination, canaries before and after it.
struct buffers {
  const std::vector<uint8_t>&src, &fill;
  std::vector<uint8_t> dst;
  explicit buffers(const patterns& p) : src(p.src), fill(p.fill), dst(CANARY + MAX_OFF + SLOT + CANARY) {}
  // one copy of `bytes` from src + so to dst + CANARY + dof; "" or what went wrong
  std::string run(copy_pool& pool, size_t bytes, size_t so, size_t dof) {
    uint8_t* d = dst.data() + CANARY + dof;
    const uint8_t* s = src.data() + so;
    memset(d - CANARY, 0xC5, CANARY);
    memset(d + bytes, 0x5C, CANARY);
    memcpy(d, fill.data() + so, bytes);
    pool.copy(d, s, bytes);
    char msg[160];
    if (memcmp(d, s, bytes)) {
      size_t first = 0, bad = 0;
      for (size_t i = bytes; i-- > 0;)
        if (d[i] != s[i]) {
          first = i;
          ++bad;
        }
      snprintf(msg, sizeof msg, "%zu bytes differ, the first at %zu (%zu before the end)", bad, first, bytes - first);
      return msg;
    }
    for (size_t i = 0; i < CANARY; ++i)
      if (d[i - (ptrdiff_t)CANARY] != 0xC5 || d[bytes + i] != 0x5C) return "canary overwritten";
    return "";
  }
};

std::vector<size_t> copy_sizes() {
  std::vector<size_t> v = {0, 1, 63, 64, 65, MiB - 1, MiB, MiB + 1, SLOT,
                           // lose 4, 1, 4, 7 and 1 bytes when per = round_up_64(floor(bytes / parts)):
                           // 1,048,641 4-byte lengths; 10,913 / 43,332 / 76,135 97-byte messages;
                           // 31,841 33-byte messages
                           4194564, 1058561, 4203204, 7385095, 1050753};
  // for every part count, the smallest and the largest m at which
  // parts * 64 * m + r splits into that many parts, every r in 0..parts
  for (size_t parts = 2; parts <= THREADS; ++parts) {
    const size_t top = parts == THREADS ? SLOT : parts * MiB;
    const size_t m_lo = (parts - 1) * MiB / (parts * 64) + 1, m_hi = top / (parts * 64) - 1;
    for (size_t m : {m_lo, m_hi})
      for (size_t r = 0; r <= parts; ++r) v.push_back(parts * 64 * m + r);
  }
  return v;
}

size_t check_copies(size_t* failures) {
  copy_pool pool(THREADS);
  const patterns pat;
  buffers b(pat);
  const size_t offs[][2] = {{0, 0}, {1, 0}, {0, 3}, {1, 3}, {3, 1}};
  size_t done = 0;
  int shown = 0;
  for (size_t bytes : copy_sizes())
    for (auto& o : offs) {
      const std::string err = b.run(pool, bytes, o[0], o[1]);
      ++done;
      if (!err.empty()) {
        ++*failures;
        if (shown++ < REPORT)
          printf("copy FAIL bytes=%zu src+%zu dst+%zu parts=%zu: %s\n", bytes, o[0], o[1],
                 copy_pool_split(bytes, THREADS).parts, err.c_str());
      }
    }
  return done;
}

// ---------------------------------------------------------------- concurrent callers
size_t check_concurrent(size_t* failures) {
  constexpr size_t CALLERS = 8, COPIES = 50;
  copy_pool pool(THREADS);
  const std::vector<size_t> sizes = copy_sizes();
  const patterns pat;
  std::vector<std::string> errs(CALLERS);
  std::vector<size_t> bad(CALLERS, 0);
  std::vector<std::thread> th;
  for (size_t t = 0; t < CALLERS; ++t)
    th.emplace_back([&, t] {
      buffers b(pat);
      uint64_t x = 0x9E3779B97F4A7C15ull * (t + 1);
      for (size_t k = 0; k < COPIES; ++k) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const size_t bytes = sizes[(x >> 33) % sizes.size()];
        const std::string err = b.run(pool, bytes, (x >> 20) & 3, (x >> 24) & 3);
        if (!err.empty() && !bad[t]++) errs[t] = "bytes=" + std::to_string(bytes) + ": " + err;
      }
    });
  for (auto& x : th) x.join();
  for (size_t t = 0; t < CALLERS; ++t)
    if (bad[t]) {
      *failures += bad[t];
      printf("concurrent FAIL caller %zu, %zu copies, the first %s\n", t, bad[t], errs[t].c_str());
    }
  return CALLERS * COPIES;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "all";
  if (what != "all" && what != "split" && what != "copy" && what != "concurrent") {
    fprintf(stderr, "usage: %s [split|copy|concurrent]\n", argv[0]);
    return 2;
  }
  size_t failures = 0, split = 0, copies = 0, conc = 0;
  if (what == "all" || what == "split") split = check_split(&failures);
  if (what == "all" || what == "copy") copies = check_copies(&failures);
  if (what == "all" || what == "concurrent") conc = check_concurrent(&failures);
  printf("copy_pool_check: split=%zu copies=%zu concurrent=%zu failures=%zu %s\n", split, copies, conc, failures,
         failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
