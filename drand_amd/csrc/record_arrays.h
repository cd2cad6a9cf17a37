// The arguments of one verify call as the host layer holds them, and the one description of the record arrays
// such a call stages (host code only, no HIP calls: capi.hip includes it, and tests/record_arrays_check.hip).
#pragma once
#include <cstring>

#include "kernels.cuh"

namespace {

using namespace dgpu;

struct rows_src;  // the stored rows of a row call (capi.hip)

// A message source as the host holds it: any of the three device types
// (kernels.cuh), selected by `linked` (SRC_*).  SRC_RECORDS: its msg_src part
// is the source; SRC_LINKED: its msg_src_linked part; SRC_HALO: with_src
// builds the msg_src_halo from the msg_src part, first_round, g0 and the two
// halo pointers (host memory until stage_prepare_locked, device after).
// rows (the row entry points; nullptr for every other form): the records are
// decoded on the device from these stored rows into the context's buffers.
struct msg_src_host : msg_src_linked {
  const uint8_t* halo;
  const uint32_t* halo_len;
  rows_src* rows;
};

// Signature group and message source of one verify call.
struct verify_args {
  int scheme;
  size_t n;
  msg_src_host m;
  const uint8_t* sigs;
  size_t sig_stride;
  const uint32_t* sig_len;
  int mode;
  uint64_t seed;
};

inline msg_src_host beacon_src(const uint64_t* rounds, const uint8_t* prev, size_t prev_stride,
                               const uint32_t* prev_len, bool chained) {
  msg_src_host m{};
  m.rounds = rounds;
  m.chained = chained ? 1 : 0;
  m.prev = chained ? prev : nullptr;
  m.prev_stride = chained ? prev_stride : 0;
  m.prev_len = chained ? prev_len : nullptr;
  return m;
}

// The linked form (kernels.cuh msg_src_linked): round first_round + g, previous
// signature = the seed (copied into the source) for g = 0, else signature
// g - 1 of the call's signature array.  seed_len <= 96 (checked by the entry
// points).
inline msg_src_host linked_src(uint64_t first_round, const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len,
                               const uint8_t* seed, size_t seed_len, bool chained) {
  msg_src_host m{};
  m.linked = SRC_LINKED;
  m.first_round = first_round;
  m.chained = chained ? 1 : 0;
  if (chained) {
    m.prev = sigs;
    m.prev_stride = sig_stride;
    m.prev_len = sig_len;
    m.seed_len = (uint32_t)seed_len;
    if (seed_len) memcpy(m.seed, seed, seed_len);
  }
  return m;
}

// One shard of a linked segment (kernels.cuh msg_src_halo): first_round is the
// shard's own first round, and item 0's previous signature is the record at
// halo / halo_len (never read by an unchained source).
inline msg_src_host halo_src(uint64_t first_round, const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len,
                             const uint8_t* halo, const uint32_t* halo_len, bool chained) {
  msg_src_host m{};
  m.linked = SRC_HALO;
  m.first_round = first_round;
  m.chained = chained ? 1 : 0;
  if (chained) {
    m.prev = sigs;
    m.prev_stride = sig_stride;
    m.prev_len = sig_len;
    m.halo = halo;
    m.halo_len = halo_len;
  }
  return m;
}

inline msg_src_host raw_src(const uint8_t* msgs, size_t stride, const uint32_t* len) {
  msg_src_host m{};
  m.msgs = msgs;
  m.msg_stride = stride;
  m.msg_len = len;
  return m;
}

// The explicit records of a row call: the decoder writes them, no pointer is the caller's.
inline msg_src_host rows_records_src(rows_src* rows, size_t prev_stride, bool chained) {
  msg_src_host m = beacon_src(nullptr, nullptr, prev_stride, nullptr, chained);
  m.rows = rows;
  return m;
}

// ---------------------------------------------------------------- the record arrays of a call
// One array a host call stages.  The list (record_arrays) alone says which
// arrays a source kind has: the device buffers, the staging through the ring,
// the pageable copy, the length checks and the staged-byte count loop over it.
enum : int { REC_ROUNDS, REC_PREV, REC_PREV_LEN, REC_MSGS, REC_MSG_LEN, REC_SIGS, REC_SIG_LEN, REC_HALO, REC_HALO_LEN,
             REC_BUFS };
enum : int { PART_ONCE, PART_MSG, PART_SIG };
// the messages of a length above its stride (item index, length), here and in the data tools' entry points
constexpr const char* MSG_LEN_FMT = "msg_len[%zu]=%u > msg_stride";
constexpr const char* PREV_LEN_FMT = "prev_len[%zu]=%u > prev_stride";

struct record_array {
  size_t field;          // its pointer's offset in verify_args: the host array, rewritten to the device copy
  int buf;               // REC_*: the context buffer that backs it
  size_t item_bytes;     // bytes per item (PART_ONCE: of the one record)
  size_t pad;            // bytes the buffer holds beyond its items (the digests' one-byte over-read)
  const uint32_t* len;   // the items' lengths (host), each at most `stride`; nullptr: nothing to check
  size_t stride;
  const char* len_fmt;   // the message of a length above the stride (item index, length)
  int part;              // PART_MSG / PART_SIG: per item, in the slice's message or signature part;
                         // PART_ONCE: once per call, ahead of slice 0, not counted in the staged bytes
};

struct record_list {
  record_array e[6];
  int n = 0;
  const record_array* begin() const { return e; }
  const record_array* end() const { return e + n; }
};

// the array pointer of entry e in a (a: the call the list was made from, or a copy of it)
inline const uint8_t* record_ptr(const verify_args& a, const record_array& e) {
  const uint8_t* p;
  memcpy(&p, (const char*)&a + e.field, sizeof p);
  return p;
}
inline void record_ptr_set(verify_args& a, const record_array& e, const void* p) {
  memcpy((char*)&a + e.field, &p, sizeof p);
}

// The arrays of call a, in the order the copy stream carries them: the
// once-per-call entries, the message part, the signature part.  The linked
// forms have no message part: their records are the signature arrays.
inline record_list record_arrays(const verify_args& a) {
  const msg_src_host& m = a.m;
  record_list L;
  auto add = [&](const void* field, int buf, size_t item_bytes, int part, size_t pad = 0, const uint32_t* len = nullptr,
                 size_t stride = 0, const char* len_fmt = nullptr) {
    L.e[L.n++] = record_array{(size_t)((const char*)field - (const char*)&a), buf, item_bytes, pad, len, stride,
                              len_fmt, part};
  };
  if (m.linked) {
    if (m.linked == SRC_HALO && m.chained) {  // one record of the stride, and its length
      add(&m.halo, REC_HALO, a.sig_stride, PART_ONCE);
      add(&m.halo_len, REC_HALO_LEN, 4, PART_ONCE);
    }
  } else if (m.msgs) {
    add(&m.msgs, REC_MSGS, m.msg_stride, PART_MSG, 1, m.msg_len, m.msg_stride, MSG_LEN_FMT);
    add(&m.msg_len, REC_MSG_LEN, 4, PART_MSG);
  } else {
    add(&m.rounds, REC_ROUNDS, 8, PART_MSG);
    if (m.chained) {
      add(&m.prev, REC_PREV, m.prev_stride, PART_MSG, 1, m.prev_len, m.prev_stride, PREV_LEN_FMT);
      add(&m.prev_len, REC_PREV_LEN, 4, PART_MSG);
    }
  }
  add(&a.sigs, REC_SIGS, a.sig_stride, PART_SIG);
  add(&a.sig_len, REC_SIG_LEN, 4, PART_SIG);
  return L;
}

// The linked forms' previous signatures are the signature arrays, wherever those moved.
inline void record_aliases(verify_args& a) {
  if (a.m.linked && a.m.chained) a.m.prev = a.sigs, a.m.prev_len = a.sig_len;
}

// Staged bytes per item (dgpu_staging_stats' bytes are n times this).
inline size_t record_item_bytes(const record_list& L) {
  size_t b = 0;
  for (const record_array& e : L) b += e.part == PART_ONCE ? 0 : e.item_bytes;
  return b;
}

// The first item of [a, b) with a length above the stride; b when every length fits.
inline size_t first_long_item(const uint32_t* len, size_t a, size_t b, size_t stride) {
  while (a < b && len[a] <= stride) ++a;
  return a;
}
// ... among the entries of `part`: the entry, and the item in *item; nullptr when every length fits.
inline const record_array* record_bad_length(const record_list& L, int part, size_t a, size_t b, size_t* item) {
  for (const record_array& e : L)
    if (e.part == part && e.len && (*item = first_long_item(e.len, a, b, e.stride)) < b) return &e;
  return nullptr;
}

}  // namespace
