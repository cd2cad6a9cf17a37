// Host check of the check-chain rule and of the faulty list's scratch layout
// (drand_amd/csrc/check_rows.cuh, scratch_layouts.h): a stand-alone program,
// host code only, driven by tests/test_check_rows_host.py.
//
//   check_rows_check [--perturb]
//
// 1. check_rows_slot / check_rows_outcome against a naive restatement of the
//    loop at chain/beacon/sync_manager.go:188-222: for every visited round,
//    Get (a lookup in an ordered map of the keys), then the three branches.  Inputs:
//    hand-made windows (missing rows, Round != key, left rows, keys outside
//    the range, n = 0, count = 0, a range that ends at 2^64 - 1) and random
//    ones.  Every array is a heap block of exactly its size.
// 2. check_rows_layout, check_lists_layout and ingest_rows_layout: regions in
//    order, disjoint, aligned to their element, the last one ending at the
//    byte count; and, over a heap block of exactly layout_bytes, a host run
//    of the four kernels' index arithmetic block by block (every thread of
//    every block, the guards as the kernels have them), so the last write of
//    each kernel lands inside its region or ASan reports it.  The lists the
//    run produces must equal the naive loop's, truncated at the caps, with the
//    guard words behind each list untouched.  Counts 1, 63, 64, 65, 255, 256,
//    257, 513 and 65,537 (one above a single pass of the block-sum scan).
// --perturb: one expected faulty value is changed first; the program must
// then report exactly one failure (it compares).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#define DG_NO_KERNELS
#include "../drand_amd/csrc/scratch_layouts.h"

using namespace dgpu;

namespace {

int g_fail = 0, g_cases = 0, g_layouts = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      if (++g_fail <= 20) {           \
        fprintf(stderr, "FAIL: ");    \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
      }                               \
    }                                 \
  } while (0)

struct window {
  uint64_t first;
  size_t count;
  std::vector<uint64_t> keys, rounds;
  std::vector<uint8_t> ok, status;
};
struct lists {
  std::vector<uint64_t> pos, val, left;
};

// the loop, restated naively
lists naive(const window& w) {
  lists L;
  std::map<uint64_t, size_t> store;  // the bucket: key -> row
  for (size_t k = 0; k < w.keys.size(); ++k) store.emplace(w.keys[k], k);
  for (size_t j = 0; j < w.count; ++j) {
    const uint64_t i = w.first + j;
    const auto it = store.find(i);
    const size_t r = it == store.end() ? w.keys.size() : it->second;
    if (r == w.keys.size()) {  // Get fails: the visited round is faulty
      L.pos.push_back(j), L.val.push_back(i);
    } else if (!w.ok[r]) {  // not canonical: the caller's decoder decides
      L.left.push_back(r);
    } else if (w.status[r]) {  // VerifyBeacon fails: the stored Round
      L.pos.push_back(j), L.val.push_back(w.rounds[r]);
    }
  }
  return L;
}

// exact-size heap copies: an access past n elements is an ASan error
template <class T>
T* heap_copy(const std::vector<T>& v) {
  T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// The four kernels' index arithmetic on the host, over the layout carved from
// a block of exactly layout_bytes; the lists have `fcap` / `lcap` entries and
// two guard words each.
lists device_walk(const window& w, size_t fcap, size_t lcap, uint64_t counts[2]) {
  const size_t count = w.count, n = w.keys.size(), nblk = check_blocks(count);
  const size_t bytes = layout_bytes<check_rows_layout>(count);
  uint8_t* buf = (uint8_t*)malloc(bytes ? bytes : 1);
  check_rows_layout L = layout_at<check_rows_layout>(buf, count);
  uint64_t* keys = heap_copy(w.keys);
  uint64_t* rounds = heap_copy(w.rounds);
  uint8_t* ok = heap_copy(w.ok);
  uint8_t* status = heap_copy(w.status);
  const uint64_t GUARD = 0xA5A5A5A5A5A5A5A5ull;
  std::vector<uint64_t> fpos(fcap + 2, GUARD), fval(fcap + 2, GUARD), left(lcap + 2, GUARD);
  memset(L.map, 0xFF, count * 4);
  // k_check_map
  for (size_t b = 0; b < (n + CHECK_BLOCK - 1) / CHECK_BLOCK; ++b)
    for (size_t t = 0; t < (size_t)CHECK_BLOCK; ++t) {
      const size_t r = b * CHECK_BLOCK + t;
      uint64_t j;
      if (r < n && check_rows_slot(w.first, count, keys[r], &j)) L.map[j] = (uint32_t)r;
    }
  // k_check_classify
  for (size_t b = 0; b < nblk; ++b) {
    uint64_t f = 0, l = 0;
    for (size_t t = 0; t < (size_t)CHECK_BLOCK; ++t) {
      const size_t j = b * CHECK_BLOCK + t;
      if (j >= count) continue;
      uint64_t val;
      const int what = check_rows_outcome(w.first, j, L.map[j], n, ok, rounds, status, &val);
      L.flags[j] = (uint8_t)what;
      f += what == CHECK_FAULTY, l += what == CHECK_LEFT;
    }
    L.blk_faulty[b] = f, L.blk_left[b] = l;
  }
  // k_check_scan: passes of CHECK_BLOCK block counts with a carry
  uint64_t carry[2] = {0, 0};
  uint64_t* arr[2] = {L.blk_faulty, L.blk_left};
  for (size_t b0 = 0; b0 < nblk; b0 += CHECK_BLOCK)
    for (int a = 0; a < 2; ++a) {
      uint64_t run = carry[a];
      for (size_t t = 0; t < (size_t)CHECK_BLOCK; ++t) {
        const size_t b = b0 + t;
        if (b >= nblk) continue;
        const uint64_t own = arr[a][b];
        arr[a][b] = run;
        run += own;
      }
      carry[a] = run;
    }
  counts[0] = carry[0], counts[1] = carry[1];
  // k_check_scatter
  for (size_t b = 0; b < nblk; ++b) {
    uint64_t f = L.blk_faulty[b], l = L.blk_left[b];
    for (size_t t = 0; t < (size_t)CHECK_BLOCK; ++t) {
      const size_t j = b * CHECK_BLOCK + t;
      const int what = j < count ? L.flags[j] : CHECK_NONE;
      if (what == CHECK_NONE) continue;
      uint64_t val;
      (void)check_rows_outcome(w.first, j, L.map[j], n, ok, rounds, status, &val);
      if (what == CHECK_FAULTY) {
        if (f < fcap) fpos[f] = j, fval[f] = val;
        ++f;
      } else {
        if (l < lcap) left[l] = val;
        ++l;
      }
    }
  }
  for (size_t g = 0; g < 2; ++g)
    CHECK(fpos[fcap + g] == GUARD && fval[fcap + g] == GUARD && left[lcap + g] == GUARD, "a list was written past its cap");
  lists out;
  const size_t nf = counts[0] < fcap ? (size_t)counts[0] : fcap, nl = counts[1] < lcap ? (size_t)counts[1] : lcap;
  out.pos.assign(fpos.begin(), fpos.begin() + nf);
  out.val.assign(fval.begin(), fval.begin() + nf);
  out.left.assign(left.begin(), left.begin() + nl);
  free(buf), free(keys), free(rounds), free(ok), free(status);
  return out;
}

void compare(const char* name, const window& w, size_t fcap, size_t lcap, bool perturb) {
  ++g_cases;
  lists want = naive(w);
  uint64_t counts[2] = {0, 0};
  lists got = device_walk(w, fcap, lcap, counts);
  CHECK(counts[0] == want.pos.size() && counts[1] == want.left.size(), "%s: totals %llu %llu, want %zu %zu", name,
        (unsigned long long)counts[0], (unsigned long long)counts[1], want.pos.size(), want.left.size());
  if (want.pos.size() > fcap) want.pos.resize(fcap), want.val.resize(fcap);
  if (want.left.size() > lcap) want.left.resize(lcap);
  if (perturb && !want.val.empty()) want.val[want.val.size() / 2] ^= 1;
  CHECK(got.pos == want.pos, "%s: faulty positions differ", name);
  CHECK(got.val == want.val, "%s: faulty values differ", name);
  CHECK(got.left == want.left, "%s: left rows differ", name);
}

window random_window(std::mt19937_64& rng, uint64_t first, size_t count, double p_missing, double p_left, double p_fail,
                     double p_round) {
  window w{first, count, {}, {}, {}, {}};
  std::uniform_real_distribution<double> u(0, 1);
  auto row = [&](uint64_t key) {
    w.keys.push_back(key);
    w.rounds.push_back(u(rng) < p_round ? key + 1 + rng() % 9 : key);
    w.ok.push_back(u(rng) < p_left ? 0 : 1);
    w.status.push_back(u(rng) < p_fail ? (uint8_t)(1 + rng() % 4) : 0);
  };
  if (first > 3 && u(rng) < 0.5) row(first - 2);  // keys outside the range take no part
  for (size_t j = 0; j < count; ++j)
    if (u(rng) >= p_missing) row(first + j);
  if (first + count < UINT64_MAX - 5 && u(rng) < 0.5) row(first + count + 1);
  return w;
}

void rule_cases(bool perturb) {
  // hand-made: rounds 10..19; 12 and 19 missing; 13 fails with Round 99; 14 is
  // left (and fails: not reported); 15 is left; 16 fails; keys 5 and 25 outside
  window w{10, 10, {5, 10, 11, 13, 14, 15, 16, 17, 18, 25}, {5, 10, 11, 99, 14, 0, 16, 17, 18, 25},
           {1, 1, 1, 1, 0, 0, 1, 1, 1, 1}, {3, 0, 0, 3, 1, 1, 2, 0, 0, 3}};
  lists want = naive(w);
  CHECK((want.pos == std::vector<uint64_t>{2, 3, 6, 9}) && (want.val == std::vector<uint64_t>{12, 99, 16, 19}) &&
            (want.left == std::vector<uint64_t>{4, 5}),
        "the naive loop itself");
  compare("hand-made", w, 10, 10, perturb);
  compare("hand-made, caps 2 / 1", w, 2, 1, false);
  compare("hand-made, caps 0 / 0", w, 0, 0, false);
  compare("n = 0", window{1, 70, {}, {}, {}, {}}, 70, 0, false);
  compare("count = 0", window{1, 0, {}, {}, {}, {}}, 0, 0, false);
  compare("count = 0, a row outside", window{7, 0, {7}, {7}, {1}, {0}}, 0, 1, false);
  // the range ends at the last 64-bit round
  compare("top of the range", window{UINT64_MAX - 4, 4, {UINT64_MAX - 4, UINT64_MAX - 2, UINT64_MAX}, {1, 2, 3},
                                     {1, 1, 1}, {1, 0, 1}},
          4, 4, false);
  // duplicate keys: which row wins is unspecified, memory safety is not (the walk must stay in bounds)
  {
    window d{1, 3, {2, 2, 9, 0}, {2, 2, 9, 0}, {1, 0, 1, 1}, {0, 0, 0, 0}};
    uint64_t counts[2];
    (void)device_walk(d, 3, 4, counts);
    CHECK(counts[0] == 2, "duplicate keys: rounds 1 and 3 are missing");
  }
  std::mt19937_64 rng(20240613);
  const size_t counts[] = {1, 63, 64, 65, 255, 256, 257, 513, 65537};
  for (size_t count : counts)
    for (int rep = 0; rep < (count > 1000 ? 3 : 6); ++rep) {
      const uint64_t first = rep % 3 == 0 ? 1 : 1 + rng() % 100000;
      window rw = rep == 0 ? random_window(rng, first, count, 0, 0, 0, 0)      // no fault
                  : rep == 1 ? random_window(rng, first, count, 1, 0, 0, 0)  // every row missing
                             : random_window(rng, first, count, 0.2, 0.1, 0.2, 0.3);
      char name[64];
      snprintf(name, sizeof name, "random count=%zu rep=%d", count, rep);
      compare(name, rw, count, rw.keys.size(), false);
      if (rep >= 2) compare(name, rw, count / 3, rw.keys.size() / 50, false);
    }
}

// regions in order, disjoint, aligned, the last one ending at `bytes`
struct region {
  const char* name;
  const void* p;
  size_t bytes, align;
};
void check_regions(const char* layout, const uint8_t* base, size_t bytes, const std::vector<region>& rs) {
  ++g_layouts;
  size_t at = 0;
  for (const region& r : rs) {
    const size_t off = (size_t)((const uint8_t*)r.p - base);
    CHECK(off >= at, "%s.%s overlaps the region before it", layout, r.name);
    CHECK(off - at < r.align, "%s.%s: a gap beyond its alignment", layout, r.name);
    CHECK(off % r.align == 0, "%s.%s is not aligned to %zu", layout, r.name, r.align);
    at = off + r.bytes;
  }
  CHECK(at == bytes, "%s: the last region ends at %zu of %zu bytes", layout, at, bytes);
}

void layout_cases() {
  const size_t counts[] = {1, 63, 64, 65, 255, 256, 257, 65536, 65537};
  for (size_t count : counts) {
    const size_t nblk = check_blocks(count), bytes = layout_bytes<check_rows_layout>(count);
    CHECK(nblk == (count + 255) / 256, "check_blocks(%zu)", count);
    CHECK(bytes == 16 * nblk + 5 * count, "check_rows_layout bytes at count %zu: %zu", count, bytes);
    uint8_t* buf = (uint8_t*)malloc(bytes);
    check_rows_layout L = layout_at<check_rows_layout>(buf, count);
    check_regions("check_rows_layout", buf, bytes,
                  {{"blk_faulty", L.blk_faulty, nblk * 8, 8}, {"blk_left", L.blk_left, nblk * 8, 8},
                   {"map", L.map, count * 4, 4}, {"flags", L.flags, count, 1}});
    L.blk_faulty[0] = L.blk_faulty[nblk - 1] = L.blk_left[0] = L.blk_left[nblk - 1] = 1;
    L.map[0] = L.map[count - 1] = 2, L.flags[0] = L.flags[count - 1] = 3;
    free(buf);
    for (size_t lcap : {(size_t)0, (size_t)3}) {
      const size_t lb = layout_bytes<check_lists_layout>(count, lcap);
      uint8_t* lbuf = (uint8_t*)malloc(lb);
      check_lists_layout D = layout_at<check_lists_layout>(lbuf, count, lcap);
      check_regions("check_lists_layout", lbuf, lb,
                    {{"counts", D.counts, 16, 8}, {"faulty_pos", D.faulty_pos, count * 8, 8},
                     {"faulty_val", D.faulty_val, count * 8, 8}, {"left_rows", D.left_rows, lcap * 8, 8}});
      D.counts[1] = D.faulty_pos[count - 1] = D.faulty_val[count - 1] = 1;
      if (lcap) D.left_rows[lcap - 1] = 1;
      free(lbuf);
    }
    for (size_t packed : {(size_t)0, (size_t)1, (size_t)17, (size_t)4096}) {
      const size_t ib = layout_bytes<ingest_rows_layout>(packed, count);
      uint8_t* ibuf = (uint8_t*)malloc(ib);
      ingest_rows_layout I = layout_at<ingest_rows_layout>(ibuf, packed, count);
      check_regions("ingest_rows_layout", ibuf, ib,
                    {{"bytes", I.bytes, packed, 16}, {"off", I.off, count * 8, 8}, {"len", I.len, count * 4, 4}});
      I.off[count - 1] = 1, I.len[count - 1] = 1;
      if (packed) I.bytes[packed - 1] = 1;
      free(ibuf);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const bool perturb = argc > 1 && !strcmp(argv[1], "--perturb");
  rule_cases(perturb);
  layout_cases();
  printf("check_rows_check: cases=%d layouts=%d failures=%d %s\n", g_cases, g_layouts, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
