// Host check of the linked message source (drand_amd/csrc/kernels.cuh msg_src,
// dgpu_verify_segment): a stand-alone program, host code only, that calls the
// very helpers the kernels call (msg_digest / msg_bad_record are host and
// device functions) and the k_randomness body (sha256_bytes).  Driven by
// tests/test_segment_host.py, which writes the case file:
//
//   stride n first_round
//   seed_len seed_hex            ("-" for an empty seed)
//   m, then m slice offsets g0
//   n lines:  sig_len record_hex (exactly `stride` bytes each)
//   n lines:  expected chained digest of global item g   (hashlib)
//   n lines:  expected unchained digest of global item g (hashlib)
//   k, then k lines: len bytes_hex expected_sha256_hex
//
// For every slice offset g0 and every item i with g = g0 + i < n the linked
// source's digest must equal (a) the digest of the explicit msg_src the
// defining property builds (rounds[g] = first_round + g, prev[0] = seed,
// prev[g] = sigs[g - 1], prev_stride = sig_stride) and (b) the expected digest
// from the file; msg_bad_record must agree with the explicit source and be
// set for exactly the record after an over-long one.  Every array is a heap
// allocation of its exact size, so a read past a stride is a sanitizer error.
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
  const size_t seed_len = strtoull(next_token(f).c_str(), nullptr, 10);
  const std::vector<uint8_t> seed = unhex(next_token(f));
  if (seed.size() != seed_len || seed_len > sizeof(msg_src_linked::seed) || n == 0) {
    fprintf(stderr, "bad seed or size\n");
    return 2;
  }
  std::vector<size_t> offsets(strtoull(next_token(f).c_str(), nullptr, 10));
  for (size_t& g0 : offsets) g0 = strtoull(next_token(f).c_str(), nullptr, 10);
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

  // the explicit records of the defining property
  uint64_t* rounds = (uint64_t*)malloc(n * 8);
  uint8_t* prev = (uint8_t*)calloc(n * stride, 1);
  uint32_t* prev_len = (uint32_t*)malloc(n * 4);
  for (size_t g = 0; g < n; ++g) {
    rounds[g] = first_round + g;
    if (g == 0) {
      prev_len[0] = (uint32_t)seed_len;
      if (seed_len) memcpy(prev, seed.data(), seed_len < stride ? seed_len : stride);
    } else {
      prev_len[g] = sig_len[g - 1];
      memcpy(prev + g * stride, sigs + (g - 1) * stride, stride);
    }
  }
  size_t digests = 0, bad_seen = 0;
  for (int chained = 1; chained >= 0; --chained) {
    msg_src ex{};
    ex.rounds = rounds;
    ex.chained = chained;
    if (chained) ex.prev = prev, ex.prev_stride = stride, ex.prev_len = prev_len;
    msg_src_linked lk{};
    lk.linked = 1;
    lk.first_round = first_round;
    lk.chained = chained;
    if (chained) {
      lk.prev = sigs, lk.prev_stride = stride, lk.prev_len = sig_len;
      lk.seed_len = (uint32_t)seed_len;
      if (seed_len) memcpy(lk.seed, seed.data(), seed_len);
    }
    for (const size_t g0 : offsets) {
      msg_src_linked sl = lk;  // what src_slice makes of it: the base pointers stay, g0 moves
      sl.g0 = g0;
      for (size_t i = 0; g0 + i < n; ++i) {
        const size_t g = g0 + i;
        uint32_t got[8], exd[8];
        msg_digest(sl, i, got);
        msg_digest(ex, g, exd);
        ++digests;
        CHECK(memcmp(got, exd, sizeof got) == 0, "chained=%d g0=%zu g=%zu: linked digest != explicit digest", chained, g0,
              g);
        CHECK(same_digest(got, chained ? want_chained[g] : want_unchained[g]),
              "chained=%d g0=%zu g=%zu: linked digest != expected", chained, g0, g);
        const bool bad = msg_bad_record(sl, i);
        const bool want_bad = chained && g > 0 && (size_t)sig_len[g - 1] > stride;
        CHECK(bad == want_bad, "chained=%d g0=%zu g=%zu: msg_bad_record=%d, want %d", chained, g0, g, (int)bad,
              (int)want_bad);
        CHECK(bad == msg_bad_record(ex, g), "chained=%d g0=%zu g=%zu: msg_bad_record differs from explicit", chained,
              g0, g);
        bad_seen += bad;
        CHECK(msg_round(sl, i) == first_round + g, "g0=%zu g=%zu: round", g0, g);
      }
    }
  }
  // the k_randomness body
  const size_t k = strtoull(next_token(f).c_str(), nullptr, 10);
  size_t hashes = 0;
  for (size_t t = 0; t < k; ++t) {
    const size_t len = strtoull(next_token(f).c_str(), nullptr, 10);
    const std::vector<uint8_t> bytes = unhex(next_token(f));
    const std::vector<uint8_t> want = unhex(next_token(f));
    if (bytes.size() != len) return 2;
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(buf, bytes.data(), len);
    uint8_t* out = (uint8_t*)malloc(32);
    sha256_bytes(out, buf, (uint32_t)len);
    CHECK(want.size() == 32 && memcmp(out, want.data(), 32) == 0, "sha256_bytes of %zu bytes", len);
    ++hashes;
    free(buf);
    free(out);
  }
  fclose(f);
  free(sigs), free(sig_len), free(rounds), free(prev), free(prev_len);
  printf("segment_src_check: digests=%zu bad_records=%zu hashes=%zu failures=%d %s\n", digests, bad_seen, hashes, g_fail,
         g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
