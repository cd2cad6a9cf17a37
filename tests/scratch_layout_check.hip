// Host check of the device scratch layouts (drand_amd/csrc/scratch_layouts.h,
// scratch_carve.h, engine_layout.cuh): a stand-alone program, host code only,
// that fills the very layout structs the library carves its DevBufs with and
// calls the index functions the kernels call (host and device functions).
// Driven by tests/test_scratch_layout_host.py:
//
//   scratch_layout_check <n>
//
// For n rounds (recovery: n rounds with t in {1, 2} commitments and m in
// {1, 3} partials per round; the RLC layouts for both signature groups) and
// for every layout it checks that
//   * the regions are in order, disjoint, and the last one ends at bytes();
//     each is aligned to the widest access its kernels make;
//   * bytes() and every region offset equal the literal values of EXPECT for
//     n = 1 and n = 65 -- the values of the expressions this header replaced
//     (one `ensure(...)` and one run of pointer arithmetic per buffer);
//   * for the wave-blocked regions (lines, f, Karabina planes, park) the
//     largest word any (round < n, plane, component, limb) addresses through
//     eng_blk_off / kb_off / h2c_park_word lies inside the region: a region
//     sized per round under an index function that works in whole blocks
//     fails here (DESIGN.md 2b', the r03i fault);
//   * the first and last element of every region can be written and read
//     back.  Every buffer is a heap allocation of exactly bytes() bytes, so an
//     access past the sizing is an ASan error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define DG_NO_KERNELS  // sizes and index functions, not the kernels (no device code to link)
#include "../drand_amd/csrc/scratch_layouts.h"

using namespace dgpu;

namespace {

int g_fail = 0;
int g_layouts = 0, g_regions = 0, g_expected = 0;
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

// bytes() and the offsets of the (non-spare) regions as the replaced
// expressions gave them, for the smallest shape and one that is a multiple of
// neither block (5 rounds, 64 rounds)
struct expect_row {
  const char* key;
  size_t bytes;
  std::vector<size_t> off;
};
const expect_row EXPECT[] = {
    {"eng_kb n=1", 32505, {0, 30240, 30520, 30800, 32480, 32500}},
    {"eng_lines n=1", 228480, {0}},
    {"eng_f n=1", 6720, {0}},
    {"eng_n1 n=1", 56, {0}},
    {"h_tmp finish n=1", 65409, {0, 224, 896, 65408}},
    {"h_tmp rlc n=1", 896, {0, 224}},
    {"cof_tmp n=1", 2688, {0, 336, 560, 784, 1456, 1680, 2352}},
    {"rlc_tree g2 n=1", 1008, {0, 336, 672, 896}},
    {"rlc_fsum g2 n=1", 672, {0, 336}},
    {"rlc_conf g2 n=1", 680, {0, 336, 672, 676}},
    {"rec_part g2 n=1", 1680, {0, 336, 672, 1008, 1344}},
    {"rlc_tree g1 n=1", 504, {0, 168, 336, 448}},
    {"rlc_fsum g1 n=1", 336, {0, 168}},
    {"rlc_conf g1 n=1", 344, {0, 168, 336, 340}},
    {"rec_part g1 n=1", 1680, {0, 168, 336, 504, 672}},
    {"msm_list n=1", 68, {0, 32}},
    {"g1_points_misc n=1", 100, {0, 4}},
    {"rec_sel n=1", 256, {0, 128}},
    {"eng_kb n=65", 422565, {0, 393120, 396760, 400400, 422240, 422500}},
    {"eng_lines n=65", 2970240, {0}},
    {"eng_f n=65", 87360, {0}},
    {"eng_n1 n=65", 3640, {0}},
    {"h_tmp finish n=65", 187329, {0, 14560, 58240, 187264}},
    {"h_tmp rlc n=65", 58240, {0, 14560}},
    {"cof_tmp n=65", 174720, {0, 21840, 36400, 50960, 94640, 109200, 152880}},
    {"rlc_tree g2 n=65", 112560,
     {0, 21840, 43680, 54768, 65856, 71568, 77280, 80304, 83328, 85008, 86688, 87696, 88704, 89376, 90048, 90384,
     90720, 105280}},
    {"rlc_fsum g2 n=65", 90720,
     {0, 21840, 43680, 54768, 65856, 71568, 77280, 80304, 83328, 85008, 86688, 87696, 88704, 89376, 90048, 90384}},
    {"rlc_conf g2 n=65", 936, {0, 336, 672, 676}},
    {"rec_part g2 n=65", 109200, {0, 21840, 43680, 65520, 87360}},
    {"rlc_tree g1 n=65", 56280,
     {0, 10920, 21840, 27384, 32928, 35784, 38640, 40152, 41664, 42504, 43344, 43848, 44352, 44688, 45024, 45192,
     45360, 52640}},
    {"rlc_fsum g1 n=65", 45360,
     {0, 10920, 21840, 27384, 32928, 35784, 38640, 40152, 41664, 42504, 43344, 43848, 44352, 44688, 45024, 45192}},
    {"rlc_conf g1 n=65", 600, {0, 168, 336, 340}},
    {"rec_part g1 n=65", 109200, {0, 10920, 21840, 32760, 43680}},
    {"msm_list n=65", 4164, {0, 2080}},
    {"g1_points_misc n=65", 6500, {0, 260}},
    {"rec_sel n=65", 16640, {0, 8320}},
    {"rlc_root g2", 672, {0, 336}},
    {"msm_runs g2", 44040192, {0, 22020096}},
    {"rlc_root g1", 336, {0, 168}},
    {"msm_runs g1", 22020096, {0, 11010048}},
    {"msm_counts", 6291456, {0, 2097152, 4194304}},
    {"g1_key_misc", 256, {0, 64, 176}},
    {"g2_key_misc", 4096, {0, 1024, 2048, 3072}},
    {"pubkey_misc", 4096, {0, 128, 512, 1024}},
    {"commits_misc t=1 cb=48", 52, {0, 48}},
    {"commits_misc t=1 cb=96", 100, {0, 96}},
    {"commits_misc t=2 cb=48", 104, {0, 96}},
    {"commits_misc t=2 cb=96", 200, {0, 192}},
};

struct region {
  const char* name;
  void* p;
  size_t bytes;  // of the region
  size_t elem;   // of one element
  size_t align;  // the widest access of its kernels
  bool spare;    // slack kept from the first sizing: not in EXPECT
};
template <class T>
region reg(const char* name, T* p, size_t count, size_t align = sizeof(T), bool spare = false) {
  return region{name, p, count * sizeof(T), sizeof(T), align, spare};
}

// One buffer: a heap block of exactly `bytes`, 16-byte aligned as any device
// allocation is at least.
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

// The generic checks of one carved layout.
void check_regions(const std::string& key, const block& b, const std::vector<region>& r) {
  ++g_layouts;
  size_t end = 0;
  std::vector<size_t> offs;
  for (size_t i = 0; i < r.size(); ++i) {
    ++g_regions;
    const size_t off = (size_t)((uint8_t*)r[i].p - b.p);
    CHECK(off >= end, "%s: region %s starts at %zu inside its predecessor (ends %zu)", key.c_str(), r[i].name, off,
          end);
    CHECK(off % r[i].align == 0, "%s: region %s at %zu not aligned to %zu", key.c_str(), r[i].name, off, r[i].align);
    CHECK(off + r[i].bytes <= b.bytes, "%s: region %s ends at %zu past bytes() = %zu", key.c_str(), r[i].name,
          off + r[i].bytes, b.bytes);
    end = off + r[i].bytes;
    if (!r[i].spare) offs.push_back(off);
  }
  CHECK(end == b.bytes, "%s: the last region ends at %zu, bytes() = %zu", key.c_str(), end, b.bytes);
  // first and last element of every region: written, then all read back
  for (size_t i = 0; i < r.size(); ++i) {
    if (!r[i].bytes) continue;
    memset(r[i].p, (int)(0x10 + 2 * i), r[i].elem);
    memset((uint8_t*)r[i].p + r[i].bytes - r[i].elem, (int)(0x11 + 2 * i), r[i].elem);
  }
  for (size_t i = 0; i < r.size(); ++i) {
    if (!r[i].bytes) continue;
    const uint8_t* first = (const uint8_t*)r[i].p;
    const uint8_t* last = first + r[i].bytes - r[i].elem;
    const bool one = r[i].bytes == r[i].elem;
    CHECK(last[0] == (uint8_t)(0x11 + 2 * i) && (one || first[0] == (uint8_t)(0x10 + 2 * i)),
          "%s: region %s: first / last element overwritten by another region", key.c_str(), r[i].name);
  }
  for (const expect_row& e : EXPECT)
    if (key == e.key) {
      ++g_expected;
      CHECK(b.bytes == e.bytes, "%s: bytes() = %zu, was %zu", key.c_str(), b.bytes, e.bytes);
      CHECK(offs == e.off, "%s: region offsets changed", key.c_str());
      for (size_t i = 0; i < offs.size() && i < e.off.size(); ++i)
        CHECK(offs[i] == e.off[i], "%s: region %zu at %zu, was %zu", key.c_str(), i, offs[i], e.off[i]);
    }
}

std::string key_n(const char* name, size_t n) { return std::string(name) + " n=" + std::to_string(n); }

// The largest word of a wave-blocked region that rounds i < n address through
// eng_blk_off (planes planes of 12 components, limbs strided by ENG_WAVE_WORDS).
size_t max_blk_word(size_t n, int planes) {
  size_t mx = 0;
  for (size_t i = 0; i < n; ++i)
    for (int pl = 0; pl < planes; ++pl)
      for (int e = 0; e < 12; ++e) {
        const size_t o = eng_blk_off(i / ENG_ROUNDS_PER_BLOCK, planes, pl, (int)(i % ENG_ROUNDS_PER_BLOCK), e) +
                         (size_t)(FP_LIMBS - 1) * ENG_WAVE_WORDS;
        if (o > mx) mx = o;
      }
  return mx;
}

void check_engine(size_t n) {
  const size_t blocks = eng_blocks(n);
  CHECK(blocks * ENG_ROUNDS_PER_BLOCK >= n && (blocks - 1) * ENG_ROUNDS_PER_BLOCK < n, "eng_blocks(%zu) = %zu", n,
        blocks);
  {  // Karabina FE state
    block b(layout_bytes<eng_kb_layout>(blocks));
    const eng_kb_layout L = layout_at<eng_kb_layout>(b.p, blocks);
    const size_t capb = blocks * ENG_ROUNDS_PER_BLOCK;
    check_regions(key_n("eng_kb", n), b,
                  {reg("xbuf", L.xbuf, eng_blk_words(blocks, ENG_KB_PLANES), 8),
                   reg("pbuf", L.pbuf, eng_n1_words(capb)), reg("pre", L.pre, eng_n1_words(capb)),
                   reg("ebuf", L.ebuf, ENG_KB_NSNAP * eng_n1_words(capb)), reg("fb", L.fb, capb),
                   reg("flags", L.flags, capb)});
    size_t mx = 0;
    for (size_t i = 0; i < n; ++i)
      for (int pl = 0; pl < ENG_KB_PLANES; ++pl)
        for (int comp = 0; comp < 12; ++comp) {
          const size_t o = kb_off(i, pl, comp) + (size_t)(FP_LIMBS - 1) * ENG_WAVE_WORDS;
          if (o > mx) mx = o;
          if (comp % 2 == 0)
            CHECK(kb_off(i, pl, comp) % 2 == 0, "kb_off(%zu, %d, %d): the Fp2 pair is not 8-byte aligned", i, pl, comp);
        }
    CHECK(mx == max_blk_word(n, ENG_KB_PLANES), "kb_off and eng_blk_off disagree at n = %zu", n);
    CHECK(mx < eng_blk_words(blocks, ENG_KB_PLANES), "eng_kb n=%zu: kb_off reaches word %zu of %zu", n, mx,
          eng_blk_words(blocks, ENG_KB_PLANES));
    L.xbuf[mx] = 1;  // (inside the exact-size block, or an ASan error)
    // the per-round planes behind it are indexed [limb][capb] up to round capb - 1
    L.ebuf[(size_t)(ENG_KB_NSNAP * FP_LIMBS - 1) * capb + (n - 1)] = 1;
    L.flags[n - 1] = 1;
  }
  // the single-region engine buffers: sized by the extent beside their index function
  const struct {
    const char* name;
    int planes;
  } blocked[] = {{"eng_lines", ENG_LINE_STEPS}, {"eng_f", ENG_F_PLANES}};
  for (const auto& B : blocked) {
    block b(eng_blk_words(blocks, B.planes) * 4);
    check_regions(key_n(B.name, n), b, {reg(B.name, (uint32_t*)b.p, eng_blk_words(blocks, B.planes), 8)});
    const size_t mx = max_blk_word(n, B.planes);
    CHECK(mx < eng_blk_words(blocks, B.planes), "%s n=%zu: eng_blk_off reaches word %zu of %zu", B.name, n, mx,
          eng_blk_words(blocks, B.planes));
    ((uint32_t*)b.p)[mx] = 1;
    // k_eng_inv's prefix products alias the line buffer
    if (B.planes == ENG_LINE_STEPS)
      CHECK(eng_n1_words(n) <= eng_blk_words(blocks, B.planes), "n=%zu: the prefix products do not fit the line buffer",
            n);
  }
  {
    block b(eng_n1_words(n) * 4);
    check_regions(key_n("eng_n1", n), b, {reg("n1", (uint32_t*)b.p, eng_n1_words(n))});
  }
  CHECK(eng_bytes_per_round() == 53597, "engine bytes per round: %zu, was 53597", eng_bytes_per_round());
}

void check_hash(size_t n) {
  for (int finish = 0; finish < 2; ++finish) {
    block b(layout_bytes<h2c_tmp_layout>(n, (bool)finish));
    const h2c_tmp_layout L = layout_at<h2c_tmp_layout>(b.p, n, (bool)finish);
    std::vector<region> r{reg("u", L.u, 4 * FP_WORDS * n), reg("q", L.q, 2 * G2J_WORDS * n)};
    if (finish) {
      r.push_back(reg("park", L.park, h2c_park_words(n), 16));
      r.push_back(reg("redo", L.redo, n));
      size_t mx = 0;
      for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < PARK_SLOTS; ++k)
          for (int w = 0; w < G2J_WORDS; ++w)
            if (h2c_park_word(i, k, w) > mx) mx = h2c_park_word(i, k, w);
      CHECK(mx < h2c_park_words(n), "h_tmp n=%zu: h2c_park_word reaches word %zu of %zu", n, mx, h2c_park_words(n));
      L.park[mx] = 1;
    } else {
      CHECK(!L.park && !L.redo, "h_tmp without the finish regions still carves them");
    }
    check_regions(key_n(finish ? "h_tmp finish" : "h_tmp rlc", n), b, r);
  }
  {
    block b(layout_bytes<cof_tmp_layout>(n));
    const cof_tmp_layout L = layout_at<cof_tmp_layout>(b.p, n);
    check_regions(key_n("cof_tmp", n), b,
                  {reg("pj", L.pj, G2J_WORDS * n), reg("pa", L.pa, G2A_WORDS * n), reg("psia", L.psia, G2A_WORDS * n),
                   reg("t1", L.t1, COF_T_WORDS * n), reg("t0a", L.t0a, G2A_WORDS * n), reg("t2", L.t2, COF_T_WORDS * n),
                   reg("u", L.u, G2J_WORDS * n)});
    // the k_cof_* kernels address the planes from the base by COF_* * n
    uint32_t* const w = L.pj;
    CHECK(L.pa == w + COF_PA * n && L.psia == w + COF_PSIA * n && L.t1 == w + COF_T1 * n && L.t0a == w + COF_T0A * n &&
              L.t2 == w + COF_T2 * n && L.u == w + COF_U * n && b.bytes == COF_WORDS * n * 4,
          "cof_tmp n=%zu: the layout and the kernels' COF_* offsets disagree", n);
  }
}

std::vector<region> level_regions(const sum_levels& T, int jw) {
  static const char* const names[2] = {"P[l]", "S[l]"};
  std::vector<region> r;
  for (int l = 0; l < T.levels; ++l) {
    r.push_back(reg(names[0], T.P[l], T.sz[l] * jw));
    r.push_back(reg(names[1], T.S[l], T.sz[l] * jw));
  }
  return r;
}

void check_rlc(size_t n) {
  for (int g1 = 0; g1 < 2; ++g1) {
    const int aw = g1 ? G1A_WORDS : G2A_WORDS, jw = g1 ? G1J_WORDS : G2J_WORDS;
    const std::string g = g1 ? "g1" : "g2";
    {
      block b(layout_bytes<rlc_tree_layout>(n, aw, jw));
      const rlc_tree_layout L = layout_at<rlc_tree_layout>(b.p, n, aw, jw);
      CHECK(L.T.sz[0] == n && L.T.sz[L.T.top()] == 1, "rlc_tree n=%zu: levels from n to the root", n);
      for (int l = 0; l < L.T.top(); ++l)
        CHECK(L.T.sz[l + 1] == (L.T.sz[l] + 1) / 2, "rlc_tree n=%zu: level %d", n, l + 1);
      std::vector<region> r = level_regions(L.T, jw);
      r.push_back(reg("rpts", L.rpts, n * aw));
      r.push_back(reg("rz", L.rz, n * (jw - aw)));
      check_regions(key_n(("rlc_tree " + g).c_str(), n), b, r);
    }
    {
      block b(layout_bytes<sum_levels>(n, jw));
      const sum_levels L = layout_at<sum_levels>(b.p, n, jw);
      check_regions(key_n(("rlc_fsum " + g).c_str(), n), b, level_regions(L, jw));
      CHECK(L.S[L.top()] == L.P[L.top()] + jw, "rlc_fsum n=%zu: the root's P and S are one stride-1 pair", n);
    }
    {
      block b(layout_bytes<rlc_conf_layout>(n, jw));
      const rlc_conf_layout L = layout_at<rlc_conf_layout>(b.p, n, jw);
      check_regions(key_n(("rlc_conf " + g).c_str(), n), b,
                    {reg("P", L.root.P, jw), reg("S", L.root.S, jw), reg("count", L.count, 1), reg("list", L.list, n)});
    }
    {
      block b(layout_bytes<rlc_root_layout>(jw));
      const rlc_root_layout L = layout_at<rlc_root_layout>(b.p, jw);
      check_regions("rlc_root " + g, b, {reg("P", L.P, jw), reg("S", L.S, jw)});
    }
    {
      block b(layout_bytes<msm_runs_layout>(jw));
      const msm_runs_layout L = layout_at<msm_runs_layout>(b.p, jw);
      const size_t words = (size_t)MSM_MW * MSM_RUNS * jw;
      check_regions("msm_runs " + g, b, {reg("runs", L.runs, words), reg("runs2", L.runs2, words)});
    }
    {
      block b(layout_bytes<rec_part_layout>(n, jw));
      const rec_part_layout L = layout_at<rec_part_layout>(b.p, n, jw);
      std::vector<region> r;
      for (int i = 0; i < rec_part_layout::SLICES; ++i) {
        r.push_back(reg("slice", L.slice[i], n * jw));
        CHECK(L.slice[i] == L.slice[0] + (size_t)i * jw * n, "rec_part n=%zu: slice %d is not at part + i * jw * n", n,
              i);
      }
      r.push_back(reg("spare", L.spare, n * rec_part_layout::SLICES * (G2J_WORDS - jw), 4, true));
      check_regions(key_n(("rec_part " + g).c_str(), n), b, r);
    }
  }
  {
    block b(layout_bytes<msm_counts_layout>());
    const msm_counts_layout L = layout_at<msm_counts_layout>(b.p);
    check_regions("msm_counts", b,
                  {reg("counts", L.counts, MSM_KEYS), reg("offsets", L.offsets, MSM_KEYS),
                   reg("cursor", L.cursor, MSM_KEYS)});
  }
  {
    block b(layout_bytes<msm_list_layout>(n));
    const msm_list_layout L = layout_at<msm_list_layout>(b.p, n);
    check_regions(key_n("msm_list", n), b,
                  {reg("list", L.list, MSM_MW * n), reg("keys", L.keys, MSM_MW * n),
                   reg("spare", L.spare, 1, 4, true)});
  }
}

void check_misc_and_recovery(size_t n) {
  {
    block b(layout_bytes<g1_key_misc>());
    const g1_key_misc L = layout_at<g1_key_misc>(b.p);
    check_regions("g1_key_misc", b, {reg("in", L.in, 64), reg("out", L.out, 2 * FP_LIMBS), reg("rc", L.rc, 20)});
    CHECK((uint32_t*)L.rc == L.out + 2 * FP_LIMBS, "g1_key_misc: rc follows out (one host copy reads both)");
  }
  {
    block b(layout_bytes<g2_key_misc>());
    const g2_key_misc L = layout_at<g2_key_misc>(b.p);
    check_regions("g2_key_misc", b,
                  {reg("pk", L.pk, 256), reg("g2", L.g2, 256), reg("rc", L.rc, 256), reg("in", L.in, 1024)});
  }
  {
    block b(layout_bytes<pubkey_misc>());
    const pubkey_misc L = layout_at<pubkey_misc>(b.p);
    check_regions("pubkey_misc", b,
                  {reg("in", L.in, 128), reg("pt", L.pt, 96), reg("rc", L.rc, 128), reg("xy", L.xy, 3072)});
  }
  for (size_t m : {(size_t)1, (size_t)3}) {  // items = n rounds x m partials
    const size_t items = n * m;
    block b(layout_bytes<g1_points_misc>(items));
    const g1_points_misc L = layout_at<g1_points_misc>(b.p, items);
    check_regions(key_n("g1_points_misc", items), b, {reg("rc", L.rc, items), reg("xy", L.xy, 96 * items)});
  }
  for (size_t t : {(size_t)1, (size_t)2})
    for (size_t cb : {(size_t)48, (size_t)96}) {
      block b(layout_bytes<commits_misc>(t, cb));
      const commits_misc L = layout_at<commits_misc>(b.p, t, cb);
      check_regions("commits_misc t=" + std::to_string(t) + " cb=" + std::to_string(cb), b,
                    {reg("in", L.in, t * cb), reg("rc", L.rc, t)});
    }
  {
    block b(layout_bytes<rec_sel_layout>(n));
    const rec_sel_layout L = layout_at<rec_sel_layout>(b.p, n);
    check_regions(key_n("rec_sel", n), b, {reg("sel", L.sel, n * RECOVER_MAX_T), reg("xs", L.xs, n * RECOVER_MAX_T)});
    for (size_t t : {(size_t)1, (size_t)2}) L.xs[(n - 1) * RECOVER_MAX_T + t - 1] = 1;  // k_recover_select's last write
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <n>\n", argv[0]);
    return 2;
  }
  const size_t n = strtoull(argv[1], nullptr, 10);
  if (n == 0) return 2;
  // the sizing pass and the carving pass of one fill() agree by construction; the carver's own rules:
  carver c{nullptr};
  CHECK(c.take<uint8_t>(3) == nullptr && c.take<uint32_t>(1) == nullptr && c.bytes() == 8,
        "carver: 3 bytes, then a word at 4");
  CHECK(c.take<uint8_t>(1, 16) == nullptr && c.bytes() == 17, "carver: explicit alignment");
  check_engine(n);
  check_hash(n);
  check_rlc(n);
  check_misc_and_recovery(n);
  printf("scratch_layout_check: n=%zu layouts=%d regions=%d expected=%d failures=%d %s\n", n, g_layouts, g_regions,
         g_expected, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
