// Host check of the halo message source (drand_amd/csrc/kernels.cuh
// msg_src_halo, dgpu_verify_segment_shard_device): a stand-alone program, host
// code only, that calls the very helpers the kernels call (msg_digest /
// msg_bad_record / msg_round are host and device functions).  Driven by
// tests/test_halo_src_host.py, which writes the case file:
//
//   stride n first_round
//   halo_len halo_hex            (min(halo_len, stride) bytes; "-" for none)
//   m, then m slice offsets g0
//   n lines:  sig_len record_hex (exactly `stride` bytes each)
//   n lines:  expected chained digest of global item g   (hashlib)
//   n lines:  expected unchained digest of global item g (hashlib)
//
// For every slice offset g0 and every item i with g = g0 + i < n the halo
// source's digest must equal (a) the digest of the explicit msg_src on the
// shifted records (rounds[g] = first_round + g, prev[0] = halo, prev_len[0] =
// halo_len, prev[g] = sigs[g - 1], prev_stride = sig_stride) and (b) the
// expected digest from the file; msg_bad_record must agree with the explicit
// source and be set for exactly item 0 under an over-long halo and the item
// after an over-long record.  Every array is a heap allocation of its exact
// size -- the halo min(halo_len, stride) bytes, its length one uint32 -- so a
// read past the halo or a stride is a sanitizer error.  The unchained pass
// hands the source null halo pointers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define DG_NO_KERNELS  // the message-source helpers, not the kernels (no device code to link)
#include "../drand_amd/csrc/kernels.cuh"

using namespace dgpu;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++g_fail;                       \
      fprintf(stderr, "FAIL: ");      \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
    }                                 \
  } while (0)

std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

std::string next_token(FILE* f) {
  std::string s;
  int ch;
  while ((ch = fgetc(f)) != EOF && (ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t')) {
  }
  for (; ch != EOF && ch != ' ' && ch != '\n' && ch != '\r' && ch != '\t'; ch = fgetc(f)) s.push_back((char)ch);
  if (s.empty()) {
    fprintf(stderr, "case file truncated\n");
    exit(2);
  }
  return s;
}

bool same_digest(const uint32_t w[8], const std::vector<uint8_t>& be32) {
  if (be32.size() != 32) return false;
  for (int k = 0; k < 8; ++k) {
    const uint32_t v = (uint32_t)be32[4 * k] << 24 | (uint32_t)be32[4 * k + 1] << 16 | (uint32_t)be32[4 * k + 2] << 8 |
                       (uint32_t)be32[4 * k + 3];
    if (v != w[k]) return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <case file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const size_t stride = strtoull(next_token(f).c_str(), nullptr, 10);
  const size_t n = strtoull(next_token(f).c_str(), nullptr, 10);
  const uint64_t first_round = strtoull(next_token(f).c_str(), nullptr, 10);
  const size_t halo_len_v = strtoull(next_token(f).c_str(), nullptr, 10);
  const std::vector<uint8_t> halo_bytes = unhex(next_token(f));
  const size_t halo_held = halo_len_v < stride ? halo_len_v : stride;
  if (halo_bytes.size() != halo_held || n == 0) {
    fprintf(stderr, "bad halo or size\n");
    return 2;
  }
  std::vector<size_t> offsets(strtoull(next_token(f).c_str(), nullptr, 10));
  for (size_t& g0 : offsets) g0 = strtoull(next_token(f).c_str(), nullptr, 10);
  // the halo: exactly the bytes its contract lets the source read, and its length
  uint8_t* halo = (uint8_t*)malloc(halo_held ? halo_held : 1);
  if (halo_held) memcpy(halo, halo_bytes.data(), halo_held);
  uint32_t* halo_len = (uint32_t*)malloc(4);
  *halo_len = (uint32_t)halo_len_v;
  // the signature arrays, each exactly as large as its contract says
  uint8_t* sigs = (uint8_t*)malloc(n * stride);
  uint32_t* sig_len = (uint32_t*)malloc(n * 4);
  for (size_t g = 0; g < n; ++g) {
    sig_len[g] = (uint32_t)strtoull(next_token(f).c_str(), nullptr, 10);
    const std::vector<uint8_t> rec = unhex(next_token(f));
    if (rec.size() != stride) {
      fprintf(stderr, "record %zu: %zu bytes\n", g, rec.size());
      return 2;
    }
    memcpy(sigs + g * stride, rec.data(), stride);
  }
  std::vector<std::vector<uint8_t>> want_chained(n), want_unchained(n);
  for (size_t g = 0; g < n; ++g) want_chained[g] = unhex(next_token(f));
  for (size_t g = 0; g < n; ++g) want_unchained[g] = unhex(next_token(f));
  fclose(f);

  // the explicit records of the defining property (the shifted records)
  uint64_t* rounds = (uint64_t*)malloc(n * 8);
  uint8_t* prev = (uint8_t*)calloc(n * stride, 1);
  uint32_t* prev_len = (uint32_t*)malloc(n * 4);
  for (size_t g = 0; g < n; ++g) {
    rounds[g] = first_round + g;
    if (g == 0) {
      prev_len[0] = (uint32_t)halo_len_v;
      if (halo_held) memcpy(prev, halo, halo_held);
    } else {
      prev_len[g] = sig_len[g - 1];
      memcpy(prev + g * stride, sigs + (g - 1) * stride, stride);
    }
  }
  size_t digests = 0, bad_seen = 0, bad_halo = 0;
  for (int chained = 1; chained >= 0; --chained) {
    msg_src ex{};
    ex.rounds = rounds;
    ex.chained = chained;
    if (chained) ex.prev = prev, ex.prev_stride = stride, ex.prev_len = prev_len;
    msg_src_halo hs{};
    hs.first_round = first_round;
    hs.chained = chained;
    if (chained) {  // (an unchained source keeps null halo pointers: it must never touch them)
      hs.prev = sigs, hs.prev_stride = stride, hs.prev_len = sig_len;
      hs.halo = halo, hs.halo_len = halo_len;
    }
    for (const size_t g0 : offsets) {
      msg_src_halo sl = hs;  // what src_slice makes of it: the base pointers stay, g0 moves
      sl.g0 = g0;
      for (size_t i = 0; g0 + i < n; ++i) {
        const size_t g = g0 + i;
        uint32_t got[8], exd[8];
        msg_digest(sl, i, got);
        msg_digest(ex, g, exd);
        ++digests;
        CHECK(memcmp(got, exd, sizeof got) == 0, "chained=%d g0=%zu g=%zu: halo digest != explicit digest", chained, g0,
              g);
        CHECK(same_digest(got, chained ? want_chained[g] : want_unchained[g]),
              "chained=%d g0=%zu g=%zu: halo digest != expected", chained, g0, g);
        const bool bad = msg_bad_record(sl, i);
        const bool want_bad =
            chained && (g == 0 ? halo_len_v > stride : (size_t)sig_len[g - 1] > stride);
        CHECK(bad == want_bad, "chained=%d g0=%zu g=%zu: msg_bad_record=%d, want %d", chained, g0, g, (int)bad,
              (int)want_bad);
        CHECK(bad == msg_bad_record(ex, g), "chained=%d g0=%zu g=%zu: msg_bad_record differs from explicit", chained,
              g0, g);
        bad_seen += bad;
        bad_halo += bad && g == 0;
        CHECK(msg_round(sl, i) == first_round + g, "g0=%zu g=%zu: round", g0, g);
      }
    }
  }
  free(halo), free(halo_len), free(sigs), free(sig_len), free(rounds), free(prev), free(prev_len);
  printf("halo_src_check: digests=%zu bad_records=%zu bad_halo=%zu failures=%d %s\n", digests, bad_seen, bad_halo,
         g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
