// Host check of k_h2c_finish's park region (drand_amd/csrc/kernels.cuh
// h2c_park_word, h2c_park_words, h2c_finish_stash): a stand-alone program,
// host code only, that calls the very helpers the kernel calls (they are host
// and device functions).  Driven by tests/test_park_layout_host.py:
//
//   park_layout_check <n> <seed>
//
// For n rounds it checks that
//   * the word offsets of all (round, slot, word) are distinct and lie below
//     the sizing expression h2c_park_words(n);
//   * every quad (words 4q .. 4q + 3) is four consecutive words starting at a
//     multiple of four, so a 16-byte aligned base gives 16-byte aligned quads;
//   * points put into the slots of every round come back exactly through
//     get(k) and through at(k).x() / y() / z(), after every slot of every
//     round has been written, and each stored word sits at h2c_park_word of
//     w = coord * 28 + comp * 14 + limb.
// The region is a heap allocation of exactly h2c_park_words(n) words, 16-byte
// aligned, so an access past the sizing expression is an ASan error and a
// misaligned quad access a UBSan error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define DG_NO_KERNELS  // the helpers, not the kernels (no device code to link)
#include "../drand_amd/csrc/kernels.cuh"

using namespace dgpu;

namespace {

int g_fail = 0;
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

uint64_t g_state;
uint32_t next_word() {  // SplitMix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// word w = coord * 28 + comp * 14 + limb of a point
uint32_t& point_word(g2j& p, int w) {
  fp2& c = w / 28 == 0 ? p.x : w / 28 == 1 ? p.y : p.z;
  fp& f = (w % 28) / 14 == 0 ? c.c0 : c.c1;
  return f.l[w % 14];
}

bool same_fp2(const fp2& a, const fp2& b) {
  return memcmp(a.c0.l, b.c0.l, sizeof a.c0.l) == 0 && memcmp(a.c1.l, b.c1.l, sizeof a.c1.l) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <n> <seed>\n", argv[0]);
    return 2;
  }
  const size_t n = strtoull(argv[1], nullptr, 10);
  g_state = strtoull(argv[2], nullptr, 10);
  if (n == 0) return 2;
  static_assert(G2J_WORDS == 84 && PARK_QUADS * 4 == G2J_WORDS, "84 words per point, 21 quads");
  const size_t words = h2c_park_words(n);
  CHECK(words == (n + 63) / 64 * 64 * 252, "h2c_park_words(%zu) = %zu: not whole 64-round blocks of 1008 B", n, words);

  // offsets: distinct, inside the region, quads consecutive and aligned
  std::vector<uint8_t> seen(words, 0);
  size_t offsets = 0;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < PARK_SLOTS; ++k)
      for (int w = 0; w < G2J_WORDS; ++w) {
        const size_t o = h2c_park_word(i, k, w);
        ++offsets;
        if (o >= words) {
          CHECK(false, "round %zu slot %d word %d: offset %zu >= %zu", i, k, w, o, words);
          continue;
        }
        CHECK(!seen[o], "round %zu slot %d word %d: offset %zu used twice", i, k, w, o);
        seen[o] = 1;
        if (w % 4 == 0)
          CHECK(o % 4 == 0, "round %zu slot %d quad %d: offset %zu is not 16-byte aligned", i, k, w / 4, o);
        else
          CHECK(o == h2c_park_word(i, k, w - 1) + 1, "round %zu slot %d word %d: not next to word %d", i, k, w, w - 1);
      }

  // put / get through a region of exactly the sizing expression
  uint32_t* park = (uint32_t*)aligned_alloc(16, words * 4);
  if (!park) return 2;
  memset(park, 0xA5, words * 4);
  std::vector<g2j> pts(n * PARK_SLOTS);
  for (g2j& p : pts)
    for (int w = 0; w < G2J_WORDS; ++w) point_word(p, w) = next_word();
  for (int k = PARK_SLOTS - 1; k >= 0; --k)  // every slot of every round, before any is read
    for (size_t i = 0; i < n; ++i) {
      h2c_finish_stash st{park, i};
      st.put(k, pts[i * PARK_SLOTS + k]);
    }
  size_t points = 0;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < PARK_SLOTS; ++k) {
      g2j& want = pts[i * PARK_SLOTS + k];
      const h2c_finish_stash st{park, i};
      const g2j got = st.get(k);
      CHECK(same_fp2(got.x, want.x) && same_fp2(got.y, want.y) && same_fp2(got.z, want.z),
            "round %zu slot %d: get differs from put", i, k);
      const auto f = st.at(k);
      CHECK(same_fp2(f.x(), want.x) && same_fp2(f.y(), want.y) && same_fp2(f.z(), want.z),
            "round %zu slot %d: at().x/y/z differ from put", i, k);
      for (int w = 0; w < G2J_WORDS; ++w)
        CHECK(park[h2c_park_word(i, k, w)] == point_word(want, w), "round %zu slot %d word %d: not at h2c_park_word", i,
              k, w);
      ++points;
    }
  free(park);
  printf("park_layout_check: n=%zu words=%zu offsets=%zu points=%zu failures=%d %s\n", n, words, offsets, points, g_fail,
         g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
