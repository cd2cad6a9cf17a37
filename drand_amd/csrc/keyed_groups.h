// The index rule of the per-key sums of dgpu_verify_keyed's RLC mode
// (keyed.cuh), as host and device functions: a host-only program includes
// this header alone (tests/keyed_groups_check.cpp).
//
// The records that are still undecided are listed grouped by key: counts per
// group, an exclusive scan (offsets), a scatter through per-group cursors.
// Group g owns list positions [offsets[g], offsets[g] + counts[g]); the order
// inside a group is whatever the atomic cursors gave, which is irrelevant --
// the sums are exact group elements.
//
// The list of L entries is cut into T = ceil(L / R) ranges of R entries (the
// last one shorter); thread t sums the runs of equal group inside range t =
// [t R, min((t + 1) R, L)), so every thread makes at most R additions whatever
// the group sizes are.  A run [s, e) of group g inside range t is
//   KEYED_RUN_WHOLE  the whole group (s <= off, e >= off + cnt): the group's sum
//   KEYED_RUN_HEAD   cut by the range's start (s > off): partial sum A[t]
//   KEYED_RUN_TAIL   cut by the range's end only: partial sum B[t]
// with at most one A and one B per range.  The fix-up joins a group that
// spans the ranges t0 < t1: sum = B[t0] + A[t0 + 1] + ... + A[t1]; a group
// inside one range was written whole; an empty group is the identity.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef DG_FN
#define DG_FN __host__ __device__ __forceinline__
#endif

namespace dgpu {

constexpr size_t KEYED_RANGE_DEFAULT = 64;  // list entries per thread of the sums
constexpr size_t KEYED_RANGES_MAX = 16384;  // ... lengthened so that a call has at most this many ranges
constexpr int KEYED_SCAN_THREADS = 1024;    // the scan's one block

enum { KEYED_RUN_WHOLE = 0, KEYED_RUN_HEAD = 1, KEYED_RUN_TAIL = 2 };

// The range length of a call of n records under the knob's value.
DG_FN size_t keyed_range_len(size_t n, size_t knob) {
  const size_t need = (n + KEYED_RANGES_MAX - 1) / KEYED_RANGES_MAX;
  const size_t r = knob ? knob : KEYED_RANGE_DEFAULT;
  return r > need ? r : need;
}

// Ranges of a list of at most n entries (the launch's thread count; the part
// buffers' extent).
DG_FN size_t keyed_ranges(size_t n, size_t R) { return n ? (n + R - 1) / R : 1; }

// The run [s, e) of a group that owns [off, off + cnt).
DG_FN int keyed_run_kind(size_t s, size_t e, size_t off, size_t cnt) {
  if (s <= off && e >= off + cnt) return KEYED_RUN_WHOLE;
  return s > off ? KEYED_RUN_HEAD : KEYED_RUN_TAIL;
}

// The ranges holding a non-empty group's first and last entries; true when
// they differ (the fix-up joins B[*t0], A[*t0 + 1 .. *t1]).
DG_FN bool keyed_group_split(size_t off, size_t cnt, size_t R, size_t* t0, size_t* t1) {
  *t0 = off / R;
  *t1 = (off + cnt - 1) / R;
  return *t0 != *t1;
}

// Groups per scan thread: the one block covers n_groups in consecutive runs.
DG_FN size_t keyed_scan_per(size_t n_groups) { return (n_groups + KEYED_SCAN_THREADS - 1) / KEYED_SCAN_THREADS; }

}  // namespace dgpu
