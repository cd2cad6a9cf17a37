// The faulty list of the bulk chain check, built on the device behind the row
// verification (dgpu_faulty_rounds_device, dgpu_check_rows).
//
// check_rows_outcome states once what SyncManager.CheckPastBeacons
// (chain/beacon/sync_manager.go:188-222) does with one visited round, as a
// host and device function.  The visited rounds are first + j for j in
// [0, count); the window's n stored rows carry keys[r] (the bolt key, the
// round the loop's Get asks for), row_ok[r] (the row is in Beacon.Marshal's
// canonical form and was decoded), rounds[r] (its stored Round) and status[r]
// (its verification, 0 = valid).  Position j:
//   no row with keys[r] == first + j        faulty, value first + j   (:202-210)
//   the row exists, row_ok[r] == 0          left: row r goes back to the caller,
//                                           which decodes it with its full
//                                           hexjson decoder; not in the list
//   the row exists, row_ok, status[r] != 0  faulty, value rounds[r]   (:212-214:
//                                           the stored Round, not the key)
//   otherwise                               nothing
// A row whose key lies outside [first, first + count) takes no part
// (check_rows_slot).
//
// The kernels (256-thread blocks, one position per thread):
//   k_check_map       position -> row, scattered from the keys with the range
//                     check of check_rows_slot (the map starts as all CHECK_NO_ROW)
//   k_check_classify  the outcome of every position as a flag byte, and each
//                     block's count of faulty and of left positions
//   k_check_scan      one block: the exclusive prefix sum of the block counts,
//                     256 at a time with a running carry, and the two totals
//   k_check_scatter   the ordered compaction: a position's place is its
//                     block's offset + the counts of the waves before its own
//                     + the flagged lanes before it in its wave (ballot,
//                     popcount); entries at or past a cap are not written
// The order is the ascending walk's by construction: no atomic append.
//
// A host-only program includes this header under DG_NO_KERNELS and takes the
// rule alone (tests/check_rows_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef DG_FN
#define DG_FN __host__ __device__ __forceinline__
#endif

namespace dgpu {

enum { CHECK_NONE = 0, CHECK_FAULTY = 1, CHECK_LEFT = 2 };
constexpr uint32_t CHECK_NO_ROW = 0xFFFFFFFFu;  // a map entry without a row (n < 2^32 - 1 rows per call)
constexpr int CHECK_BLOCK = 256;                // threads (positions) per block; block counts per scan pass

// The position of the row with this key, or false when the key lies outside
// the visited range [first, first + count) (first + count does not wrap).
DG_FN bool check_rows_slot(uint64_t first, uint64_t count, uint64_t key, uint64_t* j) {
  if (key < first || key - first >= count) return false;
  *j = key - first;
  return true;
}

// The outcome of position j, whose row is r (CHECK_NO_ROW, or any r >= n: no
// row): CHECK_FAULTY with the faulty value in *val, CHECK_LEFT with the row
// index in *val, or CHECK_NONE.
DG_FN int check_rows_outcome(uint64_t first, uint64_t j, uint32_t r, size_t n, const uint8_t* row_ok,
                             const uint64_t* rounds, const uint8_t* status, uint64_t* val) {
  if (r == CHECK_NO_ROW || r >= n) {
    *val = first + j;
    return CHECK_FAULTY;
  }
  if (!row_ok[r]) {
    *val = r;
    return CHECK_LEFT;
  }
  if (status[r]) {
    *val = rounds[r];
    return CHECK_FAULTY;
  }
  return CHECK_NONE;
}

// blocks of CHECK_BLOCK positions
DG_FN constexpr size_t check_blocks(size_t count) { return (count + CHECK_BLOCK - 1) / CHECK_BLOCK; }

#ifndef DG_NO_KERNELS
// ---------------------------------------------------------------- kernels
constexpr int CHECK_WAVES = CHECK_BLOCK / 64;

__global__ __launch_bounds__(CHECK_BLOCK) void k_check_map(uint64_t first, size_t count, size_t n,
                                                           const uint64_t* __restrict__ keys,
                                                           uint32_t* __restrict__ map) {
  const size_t r = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
  if (r >= n) return;
  uint64_t j;
  if (check_rows_slot(first, count, keys[r], &j)) map[j] = (uint32_t)r;
}

// the lanes of this wave whose flag equals `what`: (count in the wave, lanes below mine)
__device__ __forceinline__ void check_wave_rank(bool mine, uint32_t lane, uint32_t* total, uint32_t* below) {
  const unsigned long long b = __ballot(mine);
  *total = (uint32_t)__popcll(b);
  *below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(CHECK_BLOCK) void k_check_classify(uint64_t first, size_t count, size_t n,
                                                                const uint32_t* __restrict__ map,
                                                                const uint8_t* __restrict__ row_ok,
                                                                const uint64_t* __restrict__ rounds,
                                                                const uint8_t* __restrict__ status,
                                                                uint8_t* __restrict__ flags,
                                                                uint64_t* __restrict__ blk_faulty,
                                                                uint64_t* __restrict__ blk_left) {
  __shared__ uint32_t s_f[CHECK_WAVES], s_l[CHECK_WAVES];
  const size_t j = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int what = CHECK_NONE;
  if (j < count) {
    uint64_t val;
    what = check_rows_outcome(first, j, map[j], n, row_ok, rounds, status, &val);
    flags[j] = (uint8_t)what;
  }
  uint32_t nf, nl, below;
  check_wave_rank(what == CHECK_FAULTY, lane, &nf, &below);
  check_wave_rank(what == CHECK_LEFT, lane, &nl, &below);
  if (lane == 0) s_f[wave] = nf, s_l[wave] = nl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = 0, l = 0;
    for (int w = 0; w < CHECK_WAVES; ++w) f += s_f[w], l += s_l[w];
    blk_faulty[blockIdx.x] = f;
    blk_left[blockIdx.x] = l;
  }
}

// One block.  blk_*[b] (the counts of block b, b < nblk) become the entries
// in front of block b; counts[0], counts[1] the totals.  A pass takes
// CHECK_BLOCK block counts: an inclusive scan inside each wave by shuffles,
// the waves' sums through LDS, and the carry of the passes before.
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_scan(size_t nblk, uint64_t* __restrict__ blk_faulty,
                                                            uint64_t* __restrict__ blk_left,
                                                            uint64_t* __restrict__ counts) {
  __shared__ uint64_t s_w[2][CHECK_WAVES];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry[2] = {0, 0};
  uint64_t* const arr[2] = {blk_faulty, blk_left};
  for (size_t b0 = 0; b0 < nblk; b0 += CHECK_BLOCK) {
    const size_t b = b0 + threadIdx.x;
    uint64_t own[2], inc[2];
    for (int a = 0; a < 2; ++a) {
      own[a] = b < nblk ? arr[a][b] : 0;
      unsigned long long v = own[a];
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long u = __shfl_up(v, d);
        if (lane >= (uint32_t)d) v += u;
      }
      inc[a] = v;
      if (lane == 63) s_w[a][wave] = v;
    }
    __syncthreads();
    for (int a = 0; a < 2; ++a) {
      uint64_t before = carry[a], all = 0;
      for (int w = 0; w < CHECK_WAVES; ++w) {
        if ((uint32_t)w < wave) before += s_w[a][w];
        all += s_w[a][w];
      }
      if (b < nblk) arr[a][b] = before + inc[a] - own[a];
      carry[a] += all;
    }
    __syncthreads();  // s_w is rewritten by the next pass
  }
  if (threadIdx.x == 0) counts[0] = carry[0], counts[1] = carry[1];
}

__global__ __launch_bounds__(CHECK_BLOCK) void k_check_scatter(
    uint64_t first, size_t count, size_t n, const uint32_t* __restrict__ map, const uint8_t* __restrict__ row_ok,
    const uint64_t* __restrict__ rounds, const uint8_t* __restrict__ status, const uint8_t* __restrict__ flags,
    const uint64_t* __restrict__ blk_faulty, const uint64_t* __restrict__ blk_left, uint64_t* __restrict__ faulty_pos,
    uint64_t* __restrict__ faulty_val, size_t faulty_cap, uint64_t* __restrict__ left_rows, size_t left_cap) {
  __shared__ uint32_t s_f[CHECK_WAVES], s_l[CHECK_WAVES];
  const size_t j = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int what = j < count ? flags[j] : CHECK_NONE;
  uint32_t nf, nl, rank_f, rank_l;
  check_wave_rank(what == CHECK_FAULTY, lane, &nf, &rank_f);
  check_wave_rank(what == CHECK_LEFT, lane, &nl, &rank_l);
  if (lane == 0) s_f[wave] = nf, s_l[wave] = nl;
  __syncthreads();
  if (what == CHECK_NONE) return;
  uint64_t at = what == CHECK_FAULTY ? blk_faulty[blockIdx.x] + rank_f : blk_left[blockIdx.x] + rank_l;
  for (uint32_t w = 0; w < wave; ++w) at += what == CHECK_FAULTY ? s_f[w] : s_l[w];
  // the flag's value again (the same inputs as k_check_classify read)
  uint64_t val;
  (void)check_rows_outcome(first, j, map[j], n, row_ok, rounds, status, &val);
  if (what == CHECK_FAULTY) {
    if (at < faulty_cap) faulty_pos[at] = j, faulty_val[at] = val;
  } else if (at < left_cap) {
    left_rows[at] = val;
  }
}
#endif  // DG_NO_KERNELS

}  // namespace dgpu
