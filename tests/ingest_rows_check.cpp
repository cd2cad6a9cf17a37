// Host check of the device row parser (drand_amd/csrc/ingest_row.cuh) against
// dgpu_ingest_decode (drand_amd/csrc/ingest.cpp, linked in as the oracle).
// Stand-alone program with its own main, host code only; built by
// tests/test_ingest_rows_host.py under ASan + UBSan.
//
//   ingest_rows_check <case file> [--perturb]
// Case file: one row per line, "<sig_stride> <prev_stride> <hex of the row or ->".
// Every row is copied into a heap block of exactly its length and every output
// record into one of exactly its stride, so a read past the row or a write
// past a stride is a sanitizer error.  Both decoders start from 0xA5-filled
// outputs; ok, round, both lengths and every byte of both strides must agree.
// --perturb flips one bit of the parser's first record before comparing (the
// test of the comparison itself).
//
//   ingest_rows_check --gather
// copy_pool::gather (drand_amd/csrc/copy_pool.h), the staging of those rows:
// 20,000 scattered rows of 0..900 bytes (some of them listed with length 0,
// as an over-long row is staged) gathered by 8 threads into a heap block of
// exactly the packed size, then a run small enough for one thread, each
// compared with a serial gather.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../drand_amd/csrc/copy_pool.h"
#include "../drand_amd/csrc/ingest_row.cuh"

extern "C" size_t dgpu_ingest_decode(size_t n, const uint8_t* base, const uint64_t* val_off, const uint32_t* val_len,
                                     uint64_t* rounds, uint8_t* sigs, size_t sig_stride, uint32_t* sig_len,
                                     uint8_t* prev, size_t prev_stride, uint32_t* prev_len, uint8_t* ok);

namespace {

struct heap_bytes {  // exactly n bytes (n = 0: a one-byte block that nothing may touch is not needed: no access at all)
  uint8_t* p;
  size_t n;
  explicit heap_bytes(size_t n_, int fill = 0xA5) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) { memset(p, fill, n_ ? n_ : 1); }
  ~heap_bytes() { free(p); }
  heap_bytes(const heap_bytes&) = delete;
};

int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int gather_check() {
  copy_pool pool(8);
  size_t failures = 0;
  for (size_t n : {(size_t)20000, (size_t)300, (size_t)1}) {
    uint64_t state = 88172645463325252ull + n;
    auto rnd = [&] { return state ^= state << 13, state ^= state >> 7, state ^= state << 17, state; };
    std::vector<uint64_t> off(n), pos(n + 1);
    std::vector<uint32_t> len(n);
    uint64_t at = 0, packed = 0;
    for (size_t i = 0; i < n; ++i) {
      at += rnd() % 64;  // a gap in front of the row
      off[i] = at;
      const uint32_t l = (uint32_t)(rnd() % 901);
      at += l;
      len[i] = rnd() % 50 == 0 ? 0 : l;  // listed with no bytes
      pos[i] = packed;
      packed += len[i];
    }
    pos[n] = packed;
    heap_bytes src(at), dst(packed), want(packed);
    for (size_t k = 0; k < src.n; ++k) src.p[k] = (uint8_t)rnd();
    for (size_t i = 0; i < n; ++i)
      if (len[i]) memcpy(want.p + pos[i], src.p + off[i], len[i]);
    // the rows from `first` on, as a later piece of a call is gathered
    for (size_t first : {(size_t)0, n / 3}) {
      memset(dst.p, 0xA5, dst.n ? dst.n : 1);
      pool.gather(dst.p, src.p, off.data() + first, len.data() + first, pos.data() + first, n - first);
      if (memcmp(dst.p, want.p + pos[first], (size_t)(packed - pos[first]))) {
        ++failures;
        fprintf(stderr, "gather of %zu rows from row %zu differs\n", n, first);
      }
    }
  }
  printf("ingest_rows_check: gather failures=%zu %s\n", failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: ingest_rows_check <case file> [--perturb] | --gather\n"), 2;
  if (!strcmp(argv[1], "--gather")) return gather_check();
  const bool perturb = argc > 2 && !strcmp(argv[2], "--perturb");
  FILE* f = fopen(argv[1], "r");
  if (!f) return perror(argv[1]), 2;
  size_t rows = 0, canonical = 0, failures = 0;
  std::vector<char> line(1 << 16);
  while (fgets(line.data(), (int)line.size(), f)) {
    unsigned long ss = 0, ps = 0;
    int at = 0;
    if (sscanf(line.data(), "%lu %lu %n", &ss, &ps, &at) < 2) return fprintf(stderr, "bad line %zu\n", rows), 2;
    std::string hex(line.data() + at);
    while (!hex.empty() && (hex.back() == '\n' || hex.back() == '\r')) hex.pop_back();
    if (hex == "-") hex.clear();
    if (hex.size() % 2) return fprintf(stderr, "odd hex on line %zu\n", rows), 2;
    heap_bytes row(hex.size() / 2);
    for (size_t k = 0; k < row.n; ++k) row.p[k] = (uint8_t)(hexval(hex[2 * k]) << 4 | hexval(hex[2 * k + 1]));
    // the oracle
    heap_bytes o_sig(ss), o_prev(ps);
    uint64_t o_round = 0xA5A5A5A5A5A5A5A5ull, off = 0;
    uint32_t o_sl = 0xA5A5A5A5u, o_pl = 0xA5A5A5A5u, len = (uint32_t)row.n;
    uint8_t o_ok = 0xA5;
    dgpu_ingest_decode(1, row.p, &off, &len, &o_round, o_sig.p, ss, &o_sl, o_prev.p, ps, &o_pl, &o_ok);
    // the parser under test
    heap_bytes t_sig(ss), t_prev(ps);
    uint64_t t_round = 0x5A5A5A5A5A5A5A5Aull;
    uint32_t t_sl = 0x5A5A5A5Au, t_pl = 0x5A5A5A5Au;
    const bool t_ok = dgpu::ingest_row_decode(row.p, len, &t_round, t_sig.p, ss, &t_sl, t_prev.p, ps, &t_pl);
    if (perturb && rows == 0 && ss) t_sig.p[ss - 1] ^= 1;
    const bool same = (o_ok == 1) == t_ok && o_ok <= 1 && o_round == t_round && o_sl == t_sl && o_pl == t_pl &&
                      !memcmp(o_sig.p, t_sig.p, ss) && !memcmp(o_prev.p, t_prev.p, ps);
    if (!same) {
      ++failures;
      fprintf(stderr, "row %zu (%zu bytes, strides %lu/%lu): ok %u/%d round %llu/%llu sig_len %u/%u prev_len %u/%u\n", rows,
              row.n, ss, ps, o_ok, (int)t_ok, (unsigned long long)o_round, (unsigned long long)t_round, o_sl, t_sl, o_pl,
              t_pl);
    }
    // the in-place form the kernel uses: the fields decoded inside a copy of the row
    {
      heap_bytes copy(row.n);
      if (row.n) memcpy(copy.p, row.p, row.n);
      uint64_t r = 0;
      uint32_t pl = 0, sl = 0;
      const bool g = dgpu::ingest_row_fields(copy.p, len, copy.p, ps, nullptr, ss, &r, &pl, &sl);
      bool eq = g == t_ok;
      if (g) eq = eq && r == o_round && pl == o_pl && sl == o_sl && !memcmp(copy.p, o_prev.p, pl) && !memcmp(copy.p + pl, o_sig.p, sl);
      if (!eq) {
        ++failures;
        fprintf(stderr, "row %zu: the in-place fields differ from the oracle\n", rows);
      }
    }
    canonical += t_ok;
    ++rows;
  }
  fclose(f);
  printf("ingest_rows_check: rows=%zu canonical=%zu failures=%zu %s\n", rows, canonical, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
