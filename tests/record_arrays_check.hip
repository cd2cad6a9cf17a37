// Host check of the one description of a call's record arrays
// (drand_amd/csrc/record_arrays.h: record_arrays and its helpers, which the
// library's three staging functions loop over): a stand-alone program, host
// code only.  Driven by tests/test_record_arrays_host.py, which writes the case
// file; every expectation comes from there.  Tokens, separated by white space:
//
//   list <kind> <chained> <sig_stride> <stride2> <bytes_per_item> <k>
//        then k entries: <name> <part> <item_bytes> <pad> <len_name>
//   bad  <kind> <item> <length> <slice> <message, '~' for ' '>
//
// kind: records | raw | linked | halo; stride2 is the previous-signature stride
// (records) or the message stride (raw).  name: the verify_args field the entry
// rewrites, which must also be the context buffer that backs it (REC_*).  part:
// once | msg | sig.  len_name: the length array the entry is checked against,
// or "-".
//
// `list` builds the call with the library's own builders over heap arrays,
// asks record_arrays for its list, and compares entries, order, staged bytes per item (once-per-call entries count 0) and
// the pointer each entry reads and rewrites; the linked forms' aliases follow
// the rewritten signature arrays.  `bad` sets one length of a 17-item call
// above its stride and runs the length check over the slices [0, 8) and
// [8, 17): only <slice> fails, with the item's global index in <message>.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define DG_NO_KERNELS  // the message sources, not the kernels (no device code to link)
#include "../drand_amd/csrc/record_arrays.h"

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

bool next_token(FILE* f, std::string* s) {
  s->clear();
  int ch;
  while ((ch = fgetc(f)) != EOF && (ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t')) {
  }
  for (; ch != EOF && ch != ' ' && ch != '\n' && ch != '\r' && ch != '\t'; ch = fgetc(f)) s->push_back((char)ch);
  return !s->empty();
}
std::string need_token(FILE* f) {
  std::string s;
  if (!next_token(f, &s)) {
    fprintf(stderr, "case file truncated\n");
    exit(2);
  }
  return s;
}
size_t need_size(FILE* f) { return strtoull(need_token(f).c_str(), nullptr, 10); }

const char* const REC_NAME[REC_BUFS] = {"rounds", "prev", "prev_len", "msgs", "msg_len",
                                        "sigs",   "sig_len", "halo", "halo_len"};
const char* const PART_NAME[] = {"once", "msg", "sig"};

// One call of a source kind over heap arrays (the length arrays exactly n
// entries: a check that reads past a slice's end is a sanitizer error).
struct call {
  size_t n;
  uint64_t* rounds;
  uint8_t *prev, *msgs, *sigs, *halo;
  uint32_t *prev_len, *msg_len, *sig_len, *halo_len;
  verify_args a;
  call(const std::string& kind, bool chained, size_t n_, size_t sig_stride, size_t stride2) : n(n_) {
    rounds = (uint64_t*)calloc(n, 8);
    prev = (uint8_t*)calloc(n * stride2 + 1, 1);
    msgs = (uint8_t*)calloc(n * stride2 + 1, 1);
    sigs = (uint8_t*)calloc(n * sig_stride + 1, 1);
    halo = (uint8_t*)calloc(sig_stride + 1, 1);
    prev_len = (uint32_t*)calloc(n, 4);
    msg_len = (uint32_t*)calloc(n, 4);
    sig_len = (uint32_t*)calloc(n, 4);
    halo_len = (uint32_t*)calloc(1, 4);
    const uint8_t seed[32] = {1, 2, 3};
    msg_src_host m{};
    if (kind == "records") m = beacon_src(rounds, prev, stride2, prev_len, chained);
    else if (kind == "raw") m = raw_src(msgs, stride2, msg_len);
    else if (kind == "linked") m = linked_src(1000, sigs, sig_stride, sig_len, seed, sizeof seed, chained);
    else if (kind == "halo") m = halo_src(1000, sigs, sig_stride, sig_len, halo, halo_len, chained);
    else {
      fprintf(stderr, "unknown kind %s\n", kind.c_str());
      exit(2);
    }
    a = verify_args{chained ? 0 : 1, n, m, sigs, sig_stride, sig_len, 0, 7};
  }
  ~call() {
    free(rounds), free(prev), free(msgs), free(sigs), free(halo);
    free(prev_len), free(msg_len), free(sig_len), free(halo_len);
  }
  // the field of a.* named `name`: its offset in verify_args and the host array the builders put there
  bool field(const std::string& name, size_t* off, const void** host) const {
    const struct {
      const char* nm;
      const void* at;
      const void* arr;
    } F[] = {{"rounds", &a.m.rounds, rounds},       {"prev", &a.m.prev, prev},       {"prev_len", &a.m.prev_len, prev_len},
             {"msgs", &a.m.msgs, msgs},             {"msg_len", &a.m.msg_len, msg_len}, {"sigs", &a.sigs, sigs},
             {"sig_len", &a.sig_len, sig_len},      {"halo", &a.m.halo, halo},       {"halo_len", &a.m.halo_len, halo_len}};
    for (const auto& f : F)
      if (name == f.nm) return *off = (size_t)((const char*)f.at - (const char*)&a), *host = f.arr, true;
    return false;
  }
};

void run_list(FILE* f) {
  const std::string kind = need_token(f);
  const bool chained = need_size(f) != 0;
  const size_t sig_stride = need_size(f), stride2 = need_size(f), want_bytes = need_size(f), k = need_size(f);
  const size_t n = 17;
  call C(kind, chained, n, sig_stride, stride2);
  const record_list L = record_arrays(C.a);
  const char* tag = kind.c_str();
  CHECK((size_t)L.n == k, "%s chained=%d: %d entries, want %zu", tag, (int)chained, L.n, k);
  CHECK(record_item_bytes(L) == want_bytes, "%s chained=%d: %zu staged bytes per item, want %zu", tag, (int)chained,
        record_item_bytes(L), want_bytes);
  verify_args dev = C.a;  // what stage_prepare_locked makes of it: every entry's pointer moved, nothing else
  static uint8_t fake[REC_BUFS][8];
  int last_part = PART_ONCE;
  for (size_t j = 0; j < k; ++j) {
    const std::string name = need_token(f), part = need_token(f);
    const size_t item_bytes = need_size(f), pad = need_size(f);
    const std::string len_name = need_token(f);
    if (j >= (size_t)L.n) continue;
    const record_array& e = L.e[j];
    size_t off = 0;
    const void* host = nullptr;
    if (!C.field(name, &off, &host)) {
      fprintf(stderr, "unknown field %s\n", name.c_str());
      exit(2);
    }
    CHECK(e.field == off, "%s chained=%d entry %zu: not the field %s", tag, (int)chained, j, name.c_str());
    CHECK(e.buf >= 0 && e.buf < REC_BUFS && name == REC_NAME[e.buf], "%s chained=%d entry %zu (%s): backed by buffer %d",
          tag, (int)chained, j, name.c_str(), e.buf);
    CHECK(e.part >= 0 && e.part <= PART_SIG && part == PART_NAME[e.part], "%s chained=%d entry %zu (%s): part %d, want %s",
          tag, (int)chained, j, name.c_str(), e.part, part.c_str());
    CHECK(e.part >= last_part, "%s chained=%d entry %zu (%s): parts out of order", tag, (int)chained, j, name.c_str());
    last_part = e.part;
    CHECK(e.item_bytes == item_bytes && e.pad == pad, "%s chained=%d entry %zu (%s): %zu bytes per item + %zu, want %zu + %zu",
          tag, (int)chained, j, name.c_str(), e.item_bytes, e.pad, item_bytes, pad);
    CHECK(record_ptr(C.a, e) == host, "%s chained=%d entry %zu (%s): does not read the caller's array", tag, (int)chained,
          j, name.c_str());
    if (len_name == "-") {
      CHECK(e.len == nullptr, "%s chained=%d entry %zu (%s): has a length check", tag, (int)chained, j, name.c_str());
    } else {
      size_t loff = 0;
      const void* larr = nullptr;
      C.field(len_name, &loff, &larr);
      CHECK(e.len == larr && e.stride == stride2 && e.len_fmt && !strncmp(e.len_fmt, len_name.c_str(), len_name.size()),
            "%s chained=%d entry %zu (%s): not checked against %s and its stride", tag, (int)chained, j, name.c_str(),
            len_name.c_str());
    }
    if (e.buf >= 0 && e.buf < REC_BUFS) record_ptr_set(dev, e, fake[e.buf]);
  }
  // the rewritten call: the listed pointers moved and only they; the linked
  // forms' previous signatures are the (moved) signature arrays
  for (int b = 0; b < REC_BUFS; ++b) {
    size_t off = 0;
    const void* host = nullptr;
    C.field(REC_NAME[b], &off, &host);
    bool listed = false;
    for (const record_array& e : L) listed |= e.field == off;
    const record_array at{off, b, 0, 0, nullptr, 0, nullptr, PART_ONCE};
    CHECK(record_ptr(dev, at) == (listed ? fake[b] : record_ptr(C.a, at)), "%s chained=%d: field %s %s", tag,
          (int)chained, REC_NAME[b], listed ? "not rewritten" : "touched by another entry's rewrite");
  }
  const verify_args moved = dev;
  record_aliases(dev);
  if (C.a.m.linked && chained)
    CHECK(dev.m.prev == fake[REC_SIGS] && (const void*)dev.m.prev_len == (const void*)fake[REC_SIG_LEN],
          "%s: the aliases do not follow the signature arrays", tag);
  else
    CHECK(dev.m.prev == moved.m.prev && dev.m.prev_len == moved.m.prev_len, "%s chained=%d: aliases moved", tag,
          (int)chained);
}

void run_bad(FILE* f) {
  const std::string kind = need_token(f);
  const size_t item = need_size(f), length = need_size(f), want_slice = need_size(f);
  std::string want_msg = need_token(f);
  for (char& ch : want_msg)
    if (ch == '~') ch = ' ';
  const size_t n = 17, stride = 96, cut[3] = {0, 8, 17};
  call C(kind, true, n, stride, stride);
  for (size_t i = 0; i < n; ++i) C.prev_len[i] = C.msg_len[i] = C.sig_len[i] = (uint32_t)(i % 5 == 1 ? 0 : stride);
  (kind == "raw" ? C.msg_len : C.prev_len)[item] = (uint32_t)length;
  const record_list L = record_arrays(C.a);
  for (size_t k = 0; k < 2; ++k) {
    size_t at = ~(size_t)0;
    const record_array* e = record_bad_length(L, PART_MSG, cut[k], cut[k + 1], &at);
    CHECK(!record_bad_length(L, PART_SIG, cut[k], cut[k + 1], &at) && !record_bad_length(L, PART_ONCE, cut[k], cut[k + 1], &at),
          "%s item %zu: slice %zu fails outside its message part", kind.c_str(), item, k);
    if (k != want_slice) {
      CHECK(!e, "%s item %zu: slice %zu fails (item %zu)", kind.c_str(), item, k, at);
      continue;
    }
    CHECK(e != nullptr, "%s item %zu: slice %zu passes", kind.c_str(), item, k);
    if (!e) continue;
    char msg[128];
    snprintf(msg, sizeof msg, e->len_fmt, at, e->len[at]);
    CHECK(want_msg == msg, "%s item %zu: message '%s', want '%s'", kind.c_str(), item, msg, want_msg.c_str());
  }
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
  size_t lists = 0, bads = 0;
  std::string cmd;
  while (next_token(f, &cmd)) {
    if (cmd == "list") run_list(f), ++lists;
    else if (cmd == "bad") run_bad(f), ++bads;
    else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  fclose(f);
  printf("record_arrays_check: lists=%zu bad_lengths=%zu failures=%d %s\n", lists, bads, g_fail, g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
