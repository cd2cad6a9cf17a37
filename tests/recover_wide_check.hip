// Host check of the wide recovery path's host-callable parts
// (drand_amd/csrc/recover_wide.cuh, scratch_layouts.h): a stand-alone program,
// host code only, driven by tests/test_recover_wide_host.py.
//
//   recover_wide_check lagrange <t>   the one-inversion Lagrange steps, run
//       thread by thread as k_recover_lagrange_wide runs them (step A for every
//       segment, step B once, step C for every point), against
//       fr_lagrange_at_zero on index sets that are random, ascending,
//       descending and contain 0 and 65535: the same eight words per point
//   recover_wide_check layouts        rec_sel_wide_layout and
//       rec_tab_wide_layout: regions ordered, disjoint, aligned, ending at
//       bytes(); first and last element of every round's row written at
//       stride t (heap blocks of exactly bytes(): an access past the sizing is
//       an ASan error)
//   recover_wide_check consts         prints the header's limits and sizes
//       (drand_amd/_lib.py restates them for the Python callers)
//   recover_wide_check chunks         recw_chunk_rounds: the chunks cover every
//       round once, stay under the budget, and a round that alone exceeds the
//       budget is a chunk of one, never zero
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define DG_NO_KERNELS
#include "../drand_amd/csrc/scratch_layouts.h"
#include "../drand_amd/csrc/recover_wide.cuh"

using namespace dgpu;

namespace {

int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)              \
  do {                                \
    ++g_checks;                       \
    if (!(cond)) {                    \
      if (++g_fail <= 20) {           \
        fprintf(stderr, "FAIL: ");    \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
      }                               \
    }                                 \
  } while (0)

// The block of k_recover_lagrange_wide, its threads one after another.
void lagrange_round(const std::vector<uint32_t>& xs, std::vector<uint32_t>* words) {
  const int t = (int)xs.size();
  const int S = recw_lag_seg(t), nseg = recw_lag_nseg(t);
  CHECK(S >= 1 && S <= RECW_LAG_SEG && nseg <= RECW_LAG_THREADS && (size_t)nseg * S >= (size_t)t &&
            (size_t)(nseg - 1) * S < (size_t)t,
        "t=%d: segments %d x %d do not tile the points", t, nseg, S);
  std::vector<fr> segp(nseg), segx(nseg);
  std::vector<fr> v((size_t)nseg * RECW_LAG_SEG);
  std::vector<uint8_t> neg((size_t)nseg * RECW_LAG_SEG);
  for (int q = 0; q < nseg; ++q) {
    bool ng[RECW_LAG_SEG] = {};
    recw_lag_step_a(xs.data(), t, q, &v[(size_t)q * RECW_LAG_SEG], ng, segp.data(), segx.data());
    for (int u = 0; u < RECW_LAG_SEG; ++u) neg[(size_t)q * RECW_LAG_SEG + u] = ng[u];
  }
  recw_lag_step_b(segp.data(), segx.data(), nseg);
  words->assign((size_t)t * 8, 0);
  for (int q = 0; q < nseg; ++q) {
    bool ng[RECW_LAG_SEG];
    for (int u = 0; u < RECW_LAG_SEG; ++u) ng[u] = neg[(size_t)q * RECW_LAG_SEG + u] != 0;
    for (int u = 0; u < S && q * S + u < t; ++u)
      recw_lag_step_c(t, q, u, &v[(size_t)q * RECW_LAG_SEG], ng, segx[q], &(*words)[(size_t)(q * S + u) * 8]);
  }
}

void check_set(const char* what, const std::vector<uint32_t>& xs, int sample) {
  const int t = (int)xs.size();
  std::vector<uint32_t> got;
  lagrange_round(xs, &got);
  // every point up to t = 65; above, a spread sample (the serial form is O(t) products per point,
  // each with its own inversion)
  for (int k = 0; k < t; ++k) {
    if (t > 65 && k % sample != 0 && k != t - 1 && k != 1) continue;
    uint32_t want[8];
    fr_lagrange_at_zero(xs.data(), t, k, want);
    CHECK(memcmp(want, &got[(size_t)k * 8], 32) == 0, "lagrange %s t=%d j=%d: words differ (%08x.. vs %08x..)", what, t, k,
          got[(size_t)k * 8], want[0]);
  }
}

int run_lagrange(int t) {
  std::mt19937 rng(1000 + t);
  // distinct share indices 0..65535 -> x = index + 1
  auto draw = [&](bool ends) {
    std::vector<uint32_t> pool(65536);
    for (uint32_t i = 0; i < 65536; ++i) pool[i] = i;
    std::shuffle(pool.begin(), pool.end(), rng);
    std::vector<uint32_t> idx(pool.begin(), pool.begin() + t);
    if (ends) {
      // 0 and 65535 in the set (t = 1: 65535 alone)
      auto has = [&](uint32_t v) { return std::find(idx.begin(), idx.end(), v) != idx.end(); };
      if (!has(65535)) idx[0] = 65535;
      if (t > 1 && !has(0)) idx[idx[0] == 65535 ? 1 : 0] = 0;
    }
    for (uint32_t& x : idx) x += 1;
    return idx;
  };
  const int sample = t > 65 ? t / 7 : 1;
  std::vector<uint32_t> xs = draw(false);
  check_set("random", xs, sample);
  std::sort(xs.begin(), xs.end());
  check_set("ascending", xs, sample);
  std::reverse(xs.begin(), xs.end());
  check_set("descending", xs, sample);
  xs = draw(true);
  check_set("with 0 and 65535", xs, sample);
  std::vector<uint32_t> dense(t);  // 1..t, the production shape
  for (int k = 0; k < t; ++k) dense[k] = (uint32_t)k + 1;
  check_set("dense", dense, sample);
  printf("recover_wide_check: lagrange t=%d checks=%d failures=%d %s\n", t, g_checks, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}

struct block {
  uint8_t* p;
  size_t bytes;
  explicit block(size_t n) : p(nullptr), bytes(n) {
    if (posix_memalign((void**)&p, 16, n ? n : 1)) abort();
    memset(p, 0xA5, n);
  }
  ~block() { free(p); }
  block(const block&) = delete;
};
struct region {
  const char* name;
  uint32_t* p;
  size_t words;
};
void check_regions(const std::string& key, const block& b, const std::vector<region>& r) {
  size_t end = 0;
  for (const region& x : r) {
    const size_t off = (size_t)((uint8_t*)x.p - b.p);
    CHECK(off >= end, "%s: region %s starts at %zu inside its predecessor (ends %zu)", key.c_str(), x.name, off, end);
    CHECK(off % 4 == 0, "%s: region %s at %zu not word aligned", key.c_str(), x.name, off);
    CHECK(off + x.words * 4 <= b.bytes, "%s: region %s ends past bytes() = %zu", key.c_str(), x.name, b.bytes);
    end = off + x.words * 4;
  }
  CHECK(end == b.bytes, "%s: the last region ends at %zu, bytes() = %zu", key.c_str(), end, b.bytes);
}

int run_layouts() {
  for (size_t n : {(size_t)1, (size_t)7, (size_t)65})
    for (size_t t : {(size_t)33, (size_t)65, (size_t)129, (size_t)RECOVER_WIDE_MAX_T}) {
      const std::string key = "rec_sel_wide n=" + std::to_string(n) + " t=" + std::to_string(t);
      block b(layout_bytes<rec_sel_wide_layout>(n, t));
      CHECK(b.bytes == 2 * n * t * 4, "%s: bytes() = %zu", key.c_str(), b.bytes);
      const rec_sel_wide_layout L = layout_at<rec_sel_wide_layout>(b.p, n, t);
      check_regions(key, b, {{"sel", L.sel, n * t}, {"xs", L.xs, n * t}});
      for (size_t r = 0; r < n; ++r) {  // the walk's first and last write of every round, at stride t
        L.sel[r * t] = (uint32_t)r, L.sel[r * t + t - 1] = (uint32_t)r + 1;
        L.xs[r * t] = (uint32_t)r + 2, L.xs[r * t + t - 1] = (uint32_t)r + 3;
      }
      for (size_t r = 0; r < n; ++r)
        CHECK(L.sel[r * t] == r && L.sel[r * t + t - 1] == r + 1 && L.xs[r * t] == r + 2 && L.xs[r * t + t - 1] == r + 3,
              "%s: round %zu overwritten", key.c_str(), r);
    }
  struct grp {
    const char* name;
    int aw, jw;
    size_t term;
  };
  const grp groups[] = {{"g2", G2A_WORDS, G2J_WORDS, RECW_TERM_BYTES_G2}, {"g1", 2 * FP_WORDS, 3 * FP_WORDS, RECW_TERM_BYTES_G1}};
  for (const grp& g : groups)
    for (size_t rounds : {(size_t)1, (size_t)3})
      for (size_t t : {(size_t)33, (size_t)129}) {
        const std::string key = std::string("rec_tab_wide ") + g.name + " rounds=" + std::to_string(rounds) + " t=" + std::to_string(t);
        block b(layout_bytes<rec_tab_wide_layout>(rounds, t, g.aw, g.jw));
        // the bytes the chunk sizing counts per term are the layout's
        CHECK(b.bytes == rounds * t * g.term, "%s: bytes() = %zu, the chunk sizing counts %zu", key.c_str(), b.bytes,
              rounds * t * g.term);
        const rec_tab_wide_layout L = layout_at<rec_tab_wide_layout>(b.p, rounds, t, g.aw, g.jw);
        const size_t ne = rounds * t * 8;
        check_regions(key, b, {{"tab", L.tab, ne * g.aw}, {"tabz", L.tabz, ne * (g.jw - g.aw)}, {"pre", L.pre, ne * FP_WORDS}});
        // SoA planes of stride ne: the last entry's last word of every region
        L.tab[(size_t)(g.aw - 1) * ne + ne - 1] = 1;
        L.tabz[(size_t)(g.jw - g.aw - 1) * ne + ne - 1] = 2;
        L.pre[(size_t)(FP_WORDS - 1) * ne + ne - 1] = 3;
        L.tab[0] = L.tabz[0] = L.pre[0] = 4;
      }
  printf("recover_wide_check: layouts checks=%d failures=%d %s\n", g_checks, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}

int run_chunks() {
  const size_t terms[] = {RECW_TERM_BYTES_G2, RECW_TERM_BYTES_G1};
  const size_t budgets[] = {1, 1000, 3 * 33 * RECW_TERM_BYTES_G2, (size_t)1 << 20, RECW_TABLE_BUDGET};
  for (size_t term : terms)
    for (size_t budget : budgets)
      for (int t : {33, 65, 129, 513, RECOVER_WIDE_MAX_T})
        for (size_t rounds : {(size_t)1, (size_t)7, (size_t)1000, (size_t)100000}) {
          const size_t per = recw_chunk_rounds(t, term, budget);
          const size_t round_bytes = term * (size_t)t;
          CHECK(per >= 1, "t=%d budget=%zu: zero rounds per chunk", t, budget);
          if (round_bytes > budget)
            CHECK(per == 1, "t=%d budget=%zu: one round exceeds the budget, chunk of %zu", t, budget, per);
          else
            CHECK(per * round_bytes <= budget && (per + 1) * round_bytes > budget, "t=%d budget=%zu: chunk of %zu rounds", t,
                  budget, per);
          // the host loop of recover_msm_wide_chunks
          size_t covered = 0, chunks = 0;
          for (size_t r0 = 0; r0 < rounds; r0 += per) {
            const size_t nc = rounds - r0 < per ? rounds - r0 : per;
            CHECK(r0 == covered && nc >= 1 && nc <= per, "t=%d: chunk at %zu of %zu rounds", t, r0, nc);
            covered += nc;
            ++chunks;
          }
          CHECK(covered == rounds && chunks == (rounds + per - 1) / per, "t=%d rounds=%zu: covered %zu in %zu chunks", t,
                rounds, covered, chunks);
        }
  CHECK(recw_chunk_rounds(33, RECW_TERM_BYTES_G2, 3 * 33 * RECW_TERM_BYTES_G2) == 3, "7 rounds at t = 33: chunks of 3");
  CHECK(RECW_TERM_BYTES_G2 == 3136 && RECW_TERM_BYTES_G1 == 1792, "the documented bytes per term");
  for (int t : {33, 64, 65, 128, 129, 256, 257, 513, RECOVER_WIDE_MAX_T}) {
    const int L = recw_lanes(t);
    CHECK(L >= 2 && L <= 64 && 64 % L == 0 && (t + L - 1) / L <= (L < 64 ? 8 : 16), "t=%d: %d lanes", t, L);
  }
  printf("recover_wide_check: chunks checks=%d failures=%d %s\n", g_checks, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "lagrange")) {
    const int t = atoi(argv[2]);
    if (t < 1 || t > RECOVER_WIDE_MAX_T) return 2;
    return run_lagrange(t);
  }
  if (argc >= 2 && !strcmp(argv[1], "layouts")) return run_layouts();
  if (argc >= 2 && !strcmp(argv[1], "chunks")) return run_chunks();
  if (argc >= 2 && !strcmp(argv[1], "consts")) {  // the values drand_amd/_lib.py restates
    printf("consts: narrow_max_t=%d max_threshold=%d term_g2=%zu term_g1=%zu budget=%zu\n", RECOVER_MAX_T,
           RECOVER_WIDE_MAX_T, RECW_TERM_BYTES_G2, RECW_TERM_BYTES_G1, RECW_TABLE_BUDGET);
    return 0;
  }
  fprintf(stderr, "usage: recover_wide_check lagrange <t> | layouts | chunks | consts\n");
  return 2;
}
