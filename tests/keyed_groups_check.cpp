// Host check of the per-key sums' index rule and scratch layout
// (drand_amd/csrc/keyed_groups.h, scratch_layouts.h keyed_rlc_layout): a
// stand-alone program, host code only, driven by tests/test_keyed_groups_host.py.
//
//   keyed_groups_check [--perturb]
//
// It walks what the kernels of dgpu_verify_keyed's RLC mode do with their
// indices -- count, the one-block scan (each of its threads over
// keyed_scan_per groups), scatter through the cursors in a shuffled order
// (the atomics' order is arbitrary), the range sums with keyed_run_kind, the
// fix-up with keyed_group_split -- over a heap block of exactly layout_bytes,
// so a write outside a region's extent lands in another region (the sums then
// differ) or outside the block (ASan reports it).  Group elements are 32-bit
// integers (one word per "point"): once random values, so a member summed
// twice or dropped changes the sum, and once all ones, so the sums are the
// counts.  P and S use different values: a mix-up of the two halves shows.
// n in {1, 63, 64, 65, 257, 4099} x K in {1, 2, 300, 65536} x range lengths
// {1, 7, 64} x {random groups, all one group, all distinct groups}; a tenth of
// the records is already decided and takes no part.
// What this program shares with the kernels is the index rule alone
// (keyed_range_len, keyed_ranges, keyed_scan_per, keyed_run_kind,
// keyed_group_split) and the layout; the loops around the rule are restated
// here, so a slip in a kernel's own loop body (its emit on a key change, the
// 2 T stride of the partial slots, the fix-up's lane order) is for the GPU
// tests to catch (tests/test_gpu_keyed.py runs a group over many ranges).
// --perturb: one expected sum is changed first; the program must then report
// exactly one failure (it compares).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define DG_NO_KERNELS
#include "../drand_amd/csrc/scratch_layouts.h"
#include "../drand_amd/csrc/keyed_groups.h"

using namespace dgpu;

namespace {

int g_fail = 0, g_cases = 0;
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

struct region {
  const void* p;
  size_t bytes;
  const char* name;
};

// regions in order, disjoint, aligned to their element, the last ending at the byte count
void check_layout(const keyed_rlc_layout& K, const uint8_t* base, size_t total, size_t n, size_t ng, size_t T, size_t m) {
  const region r[] = {{K.counts, ng * 4, "counts"}, {K.offsets, ng * 4, "offsets"}, {K.cursor, ng * 4, "cursor"},
                      {K.cpos, ng * 4, "cpos"},     {K.totals, 8, "totals"},        {K.nfail, 4, "nfail"},
                      {K.list, n * 4, "list"},      {K.lkey, n * 4, "lkey"},        {K.flist, n * 4, "flist"},
                      {K.leaf_p, n * 4, "leaf_p"},  {K.leaf_s, n * 4, "leaf_s"},    {K.sums, 2 * ng * 4, "sums"},
                      {K.part, 4 * T * 4, "part"},  {K.ch, m * 4, "ch"},            {K.cs, m * 4, "cs"},
                      {K.ckeys, m * 4, "ckeys"},    {K.cst, m, "cst"}};
  size_t at = 0;
  for (const region& e : r) {
    const size_t off = (size_t)((const uint8_t*)e.p - base);
    CHECK(off == at, "%s starts at %zu, expected %zu", e.name, off, at);
    CHECK(e.p == (const void*)K.cst || off % 4 == 0, "%s misaligned", e.name);
    at = off + e.bytes;
  }
  CHECK(at == total, "the regions end at %zu of %zu bytes", at, total);
}

void run_case(size_t n, size_t ng, size_t R, int pattern, bool ones, bool perturb, std::mt19937_64& rng) {
  ++g_cases;
  const size_t T = keyed_ranges(n, R), m = std::min(ng, n);
  const size_t total = layout_bytes<keyed_rlc_layout>(n, ng, T, m, 1, 1, 1);
  uint8_t* block = (uint8_t*)malloc(total);
  memset(block, 0xA5, total);
  const keyed_rlc_layout K = layout_at<keyed_rlc_layout>(block, n, ng, T, m, 1, 1, 1);
  check_layout(K, block, total, n, ng, T, m);
  // the records: group ids, statuses (0 = undecided), leaves
  std::vector<uint32_t> gid(n);
  std::vector<uint8_t> st(n);
  for (size_t i = 0; i < n; ++i) {
    gid[i] = pattern == 0 ? (uint32_t)(rng() % ng) : pattern == 1 ? (uint32_t)(ng - 1) : (uint32_t)(i % ng);
    st[i] = rng() % 10 == 0 ? 1 : 0;
    K.leaf_p[i] = ones ? 1u : (uint32_t)rng();
    K.leaf_s[i] = ones ? 1u : (uint32_t)rng();
  }
  std::vector<uint32_t> want_p(ng, 0), want_s(ng, 0), want_c(ng, 0);
  for (size_t i = 0; i < n; ++i)
    if (!st[i]) want_p[gid[i]] += K.leaf_p[i], want_s[gid[i]] += K.leaf_s[i], want_c[gid[i]]++;
  if (perturb) want_p[gid[0]] += 1;
  // count
  for (size_t g = 0; g < ng; ++g) K.counts[g] = 0;
  for (size_t i = 0; i < n; ++i)
    if (!st[i] && gid[i] < ng) K.counts[gid[i]]++;
  // the one-block scan: thread t over keyed_scan_per(ng) consecutive groups
  {
    const size_t per = keyed_scan_per(ng);
    uint32_t run = 0, slot = 0;
    for (size_t t = 0; t < (size_t)KEYED_SCAN_THREADS; ++t) {
      const size_t g0 = t * per, g1 = std::min(g0 + per, ng);
      for (size_t g = g0; g < g1; ++g) {
        K.offsets[g] = run, K.cursor[g] = run, K.cpos[g] = slot;
        run += K.counts[g], slot += K.counts[g] != 0;
      }
    }
    K.totals[0] = run, K.totals[1] = slot;
    CHECK(per * KEYED_SCAN_THREADS >= ng, "the scan's threads do not cover %zu groups", ng);
    CHECK(slot <= m, "%u non-empty groups in %zu slots", slot, m);
  }
  // scatter, in a shuffled order
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = i;
  std::shuffle(order.begin(), order.end(), rng);
  for (size_t i : order) {
    if (st[i] || gid[i] >= ng) continue;
    const uint32_t pos = K.cursor[gid[i]]++;
    K.list[pos] = (uint32_t)i, K.lkey[pos] = gid[i];
  }
  // range sums: 2T threads
  const size_t L = K.totals[0];
  for (size_t id = 0; id < 2 * T; ++id) {
    const bool sig = id >= T;
    const size_t t = sig ? id - T : id, p0 = t * R;
    if (p0 >= L) continue;
    const size_t p1 = std::min(p0 + R, L);
    const uint32_t* leaf = sig ? K.leaf_s : K.leaf_p;
    uint32_t* gsum = K.sums + (sig ? ng : 0);
    uint32_t* gpart = K.part + (sig ? 2 * T : 0);
    auto emit = [&](uint32_t g, size_t s, size_t e, uint32_t acc) {
      const int kind = keyed_run_kind(s, e, K.offsets[g], K.counts[g]);
      if (kind == KEYED_RUN_WHOLE) gsum[g] = acc;
      else gpart[kind == KEYED_RUN_HEAD ? t : T + t] = acc;
    };
    uint32_t g = K.lkey[p0], acc = 0;
    size_t s = p0, adds = 0;
    for (size_t p = p0; p < p1; ++p) {
      if (K.lkey[p] != g) {
        emit(g, s, p, acc);
        g = K.lkey[p], s = p, acc = 0;
      }
      acc += leaf[K.list[p]];
      ++adds;
    }
    emit(g, s, p1, acc);
    CHECK(adds <= R, "range %zu made %zu additions, more than its length %zu", t, adds, R);
  }
  // fix-up: 2 ng threads
  for (size_t id = 0; id < 2 * ng; ++id) {
    const bool sig = id >= ng;
    const size_t g = sig ? id - ng : id;
    uint32_t* gsum = K.sums + (sig ? ng : 0);
    const uint32_t* gpart = K.part + (sig ? 2 * T : 0);
    if (K.counts[g] == 0) {
      gsum[g] = 0;
      continue;
    }
    size_t t0, t1;
    if (!keyed_group_split(K.offsets[g], K.counts[g], R, &t0, &t1)) continue;
    CHECK(t1 < T, "group %zu ends in range %zu of %zu", g, t1, T);
    uint32_t acc = gpart[T + t0];
    for (size_t t = t0 + 1; t <= t1; ++t) acc += gpart[t];
    gsum[g] = acc;
  }
  for (size_t g = 0; g < ng; ++g) {
    CHECK(K.counts[g] == want_c[g], "n=%zu K=%zu R=%zu: count of group %zu", n, ng, R, g);
    CHECK(K.sums[g] == want_p[g], "n=%zu K=%zu R=%zu pattern %d: P sum of group %zu is %u, expected %u", n, ng, R, pattern,
          g, K.sums[g], want_p[g]);
    CHECK(K.sums[ng + g] == want_s[g], "n=%zu K=%zu R=%zu pattern %d: S sum of group %zu", n, ng, R, pattern, g);
  }
  free(block);
}

}  // namespace

int main(int argc, char** argv) {
  const bool perturb = argc > 1 && !strcmp(argv[1], "--perturb");
  std::mt19937_64 rng(20240607);
  // the shipped range length: at most KEYED_RANGES_MAX ranges, never below the default or the knob
  CHECK(keyed_range_len(1, 0) == KEYED_RANGE_DEFAULT && keyed_range_len(1 << 20, 0) == 64 &&
            keyed_range_len((1 << 20) + 1, 0) == 65 && keyed_range_len(4099, 7) == 7 &&
            keyed_ranges(1 << 24, keyed_range_len(1 << 24, 0)) <= KEYED_RANGES_MAX,
        "keyed_range_len");
  // hand-made: a group over three ranges whose neighbours share a range
  CHECK(keyed_run_kind(4, 8, 2, 10) == KEYED_RUN_HEAD && keyed_run_kind(2, 4, 2, 10) == KEYED_RUN_TAIL &&
            keyed_run_kind(8, 12, 2, 10) == KEYED_RUN_HEAD && keyed_run_kind(0, 2, 0, 2) == KEYED_RUN_WHOLE &&
            keyed_run_kind(1, 2, 1, 1) == KEYED_RUN_WHOLE,
        "keyed_run_kind");
  {
    size_t t0, t1;
    CHECK(keyed_group_split(2, 10, 4, &t0, &t1) && t0 == 0 && t1 == 2, "keyed_group_split(2, 10, 4)");
    CHECK(!keyed_group_split(4, 4, 4, &t0, &t1) && t0 == 1 && t1 == 1, "keyed_group_split(4, 4, 4)");
  }
  bool first = true;
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)257, (size_t)4099})
    for (size_t ng : {(size_t)1, (size_t)2, (size_t)300, (size_t)65536})
      for (size_t R : {(size_t)1, (size_t)7, (size_t)64})
        for (int pattern = 0; pattern < 3; ++pattern)
          for (int ones = 0; ones < 2; ++ones) {
            run_case(n, ng, R, pattern, ones != 0, perturb && first, rng);
            first = false;
          }
  printf("keyed_groups_check: cases=%d failures=%d %s\n", g_cases, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
