// Threshold recovery for groups above RECOVER_MAX_T: the "wide" path,
// RECOVER_MAX_T < t <= RECOVER_WIDE_MAX_T (drand's key.MinimumT(n) = n/2 + 1
// puts every group of 64 nodes and more here).  The round semantics are
// recover.cuh's, word for word (its header and the comment of k_recover_cand);
// what differs is how a round's work is laid out:
//
//   * sel, xs and the digits have stride t (rec_sel_wide_layout), not 32;
//   * a block per round walks the partials (k_recover_walk_wide): ranks by
//     wave ballots, duplicates through an LDS bitmap over the 65536 possible
//     indices, no array sized by t in a thread's private memory;
//   * a block per round computes the t Lagrange coefficients with ONE Fr
//     inversion (k_recover_lagrange_wide): lambda_j = P / (x_j d_j) with
//     P = prod x_k, d_j = prod_{k != j} (x_k - x_j);
//   * L lanes per (round, slice) share the MSM's t terms
//     (k_recover_msm_wide, k_recover_rlc_wide), their partial sums added in an
//     LDS tree with the complete addition;
//   * the window tables of a batch are built in chunks of rounds under
//     RECW_TABLE_BUDGET bytes (threshold_host.h recover_msm_wide_locked).
//
// The host-callable part (above DG_NO_KERNELS) is shared with
// tests/recover_wide_check.hip, which runs the Lagrange steps thread by thread
// against fr_lagrange_at_zero.
#pragma once
#include "fr.cuh"
#include "recover.cuh"

namespace dgpu {

constexpr int RECOVER_WIDE_MAX_T = 1024;  // DGPU_MAX_THRESHOLD

// ---------------------------------------------------------------- chunking
// Window-table bytes per term: 8 entries of an affine point (X, Y), its Z
// until the batch inversion, and that inversion's prefix product.
constexpr size_t RECW_TERM_BYTES_G2 = 8 * (size_t)(G2A_WORDS + 2 * FP_WORDS + FP_WORDS) * 4;  // 3,136
constexpr size_t RECW_TERM_BYTES_G1 = 8 * (size_t)(2 * FP_WORDS + FP_WORDS + FP_WORDS) * 4;   // 1,792
// the budget of one chunk's tables
constexpr size_t RECW_TABLE_BUDGET = (size_t)1 << 30;
// Rounds per chunk: as many as fit the budget, never zero (one round alone
// above the budget is a chunk of its own).
inline size_t recw_chunk_rounds(int t, size_t term_bytes, size_t budget) {
  const size_t c = budget / (term_bytes * (size_t)t);
  return c ? c : 1;
}

// ---------------------------------------------------------------- lanes per slice
// L lanes share the t terms of one (round, slice): every lane runs the whole
// window loop (64 doublings and 17 additions per term it owns) over the terms
// j = lane, lane + L, ..., then log2 L complete additions join the lanes.
// The doublings are paid per lane whatever it owns, so L is the smallest
// power of two that leaves a lane at most 8 terms: the 17 * 8 additions then
// outweigh the 64 doublings two to one, and the chain per round is about
// 17 t / L + 64 + log2 L point operations (t = 33: 152 against the narrow
// kernels' 17 t + 64 = 625).  L stops at 64: a slice stays inside one wave,
// which is the whole block (64 threads), so the tree's barriers cost a wave
// nothing and its LDS (32 Jacobian points, 10.5 KB on G2) lets the eight
// blocks of a CU at the kernels' 2 waves per SIMD coexist (84 of 160 KB).
// At t = 1024 a lane owns 16 terms and the chain is 342.
DG_FN int recw_lanes(int t) { return t <= 64 ? 8 : t <= 128 ? 16 : t <= 256 ? 32 : 64; }

// ---------------------------------------------------------------- Lagrange, one inversion
// A block of RECW_LAG_THREADS threads per round; thread q owns the segment
// j in [q S, min(t, (q + 1) S)) with S = recw_lag_seg(t) <= RECW_LAG_SEG.
//   step A (every thread)  v_j = x_j |d_j| and the sign of d_j for its j;
//                          segp[q] = prod v_j, segx[q] = prod x_j
//   step B (thread 0)      base[q] = P / prod_{q' != q} segp[q'] ... / total:
//                          prefix and suffix products of segp around ONE
//                          fr_inv of their total, times P = prod segx
//   step C (every thread)  lambda_j = base[q] prod_{k in seg, k != j} v_k,
//                          negated for a negative d_j, canonical words
// All factors of d_j are integers below 2^17 in magnitude: three at a time
// are multiplied as integers (< 2^51) before one Fr product.
constexpr int RECW_LAG_THREADS = 256;
constexpr int RECW_LAG_SEG = RECOVER_WIDE_MAX_T / RECW_LAG_THREADS;
DG_FN int recw_lag_seg(int t) { return (t + RECW_LAG_THREADS - 1) / RECW_LAG_THREADS; }
DG_FN int recw_lag_nseg(int t) { return (t + recw_lag_seg(t) - 1) / recw_lag_seg(t); }

// integer below 2^56 -> Montgomery form
DG_FN fr recw_fr_from_u56(uint64_t x) {
  fr a{};
  a.l[0] = (uint32_t)x & FP_MASK;
  a.l[1] = (uint32_t)(x >> FP_BITS) & FP_MASK;
  return fr_mul(a, fr_from_limbs(FR_R2));
}

// x_j |d_j| (Montgomery), neg = the sign of d_j = prod_{k != j} (x_k - x_j)
DG_FN fr recw_lag_den(const uint32_t* xs, int t, int j, bool& neg) {
  const int64_t xj = (int64_t)xs[j];
  fr acc = fr_from_u32(xs[j]);
  uint64_t pend = 1;
  int np = 0;
  bool ng = false;
  for (int k = 0; k < t; ++k) {
    if (k == j) continue;
    const int64_t d = (int64_t)xs[k] - xj;
    ng ^= d < 0;
    pend *= (uint64_t)(d < 0 ? -d : d);
    if (++np == 3) {
      acc = fr_mul(acc, recw_fr_from_u56(pend));
      pend = 1;
      np = 0;
    }
  }
  if (np) acc = fr_mul(acc, recw_fr_from_u56(pend));
  neg = ng;
  return acc;
}

DG_FN void recw_lag_step_a(const uint32_t* xs, int t, int q, fr v[RECW_LAG_SEG], bool neg[RECW_LAG_SEG], fr* segp,
                           fr* segx) {
  const int S = recw_lag_seg(t);
  fr p = fr_from_limbs(FR_ONE_M), px = fr_from_limbs(FR_ONE_M);
#pragma unroll
  for (int u = 0; u < RECW_LAG_SEG; ++u) {
    const int j = q * S + u;
    if (u < S && j < t) {
      v[u] = recw_lag_den(xs, t, j, neg[u]);
      p = fr_mul(p, v[u]);
      px = fr_mul(px, fr_from_u32(xs[j]));
    }
  }
  segp[q] = p;
  segx[q] = px;
}

// segx in: the segments' products of x; out: base[q]
DG_FN void recw_lag_step_b(const fr* segp, fr* segx, int nseg) {
  fr P = fr_from_limbs(FR_ONE_M);
  for (int q = 0; q < nseg; ++q) P = fr_mul(P, segx[q]);
  fr run = fr_from_limbs(FR_ONE_M);
  for (int q = 0; q < nseg; ++q) {  // exclusive prefix products
    segx[q] = run;
    run = fr_mul(run, segp[q]);
  }
  run = fr_mul(P, fr_inv(run));  // the one inversion: v_j != 0 (distinct x, r prime)
  for (int q = nseg - 1; q >= 0; --q) {  // ... times the exclusive suffix products
    segx[q] = fr_mul(segx[q], run);
    run = fr_mul(run, segp[q]);
  }
}

// lambda of the u-th point of segment q, as fr_lagrange_at_zero's words
DG_FN void recw_lag_step_c(int t, int q, int u, const fr v[RECW_LAG_SEG], const bool neg[RECW_LAG_SEG], const fr& base,
                           uint32_t* out_words) {
  const int S = recw_lag_seg(t);
  fr l = base;
#pragma unroll
  for (int k = 0; k < RECW_LAG_SEG; ++k)
    if (k != u && k < S && q * S + k < t) l = fr_mul(l, v[k]);
  l = fr_canon(l);
  if (neg[u]) {
    bool zero = true;
    for (int i = 0; i < FR_LIMBS; ++i) zero = zero && l.l[i] == 0;
    if (!zero) l = fr_neg(l);
  }
  fr_to_words(l, out_words);
}

}  // namespace dgpu

#ifndef DG_NO_KERNELS
#include "recover_g1.cuh"
#include "group_ops.cuh"

namespace dgpu {

// ================================================================ the walk
// Exclusive rank of `pred` among the block's 256 threads (wave ballots, the
// four wave counts through LDS); total = the block's count.  Block-uniform call.
__device__ __forceinline__ int recw_block_rank(bool pred, int* s_w, int& total) {
  const unsigned long long mask = __ballot(pred);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // s_w free again
  if (lane == 0) s_w[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    before += k < wave ? s_w[k] : 0;
    all += s_w[k];
  }
  total = all;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// One block per round.  SELECT = false: k_recover_cand's classes (candidates
// = the first t ST_OK partials, duplicates included in sel); SELECT = true:
// k_recover_select after the VerifyPartial pairings (the first t good ones,
// deduplicated in input order; a failure is final).  The partials are walked
// in chunks of 256 slots; a partial's index is a duplicate when the bitmap has
// it from an earlier chunk or an earlier slot of this chunk holds it (one
// pass over the chunk's ids in LDS: O(m) per thread, not O(t^2)).
template <bool SELECT>
__global__ void __launch_bounds__(256) k_recover_walk_wide(size_t n_rounds, size_t m, int t, int want_status,
                                                           const uint32_t* __restrict__ idx,
                                                           const uint8_t* __restrict__ status,
                                                           uint32_t* __restrict__ sel, uint32_t* __restrict__ xs,
                                                           uint8_t* __restrict__ cls, uint8_t* __restrict__ ok,
                                                           uint8_t* __restrict__ out96,
                                                           const uint32_t* __restrict__ commits,
                                                           uint32_t* __restrict__ rec_pts, uint32_t* __restrict__ rec_pk,
                                                           uint8_t* __restrict__ rec_st) {
  __shared__ uint32_t s_bits[65536 / 32];
  __shared__ uint32_t s_ids[256];
  __shared__ uint8_t s_in[256];
  __shared__ int s_w[4];
  const size_t r = blockIdx.x;
  const int tid = threadIdx.x;
  for (int k = tid; k < 65536 / 32; k += 256) s_bits[k] = 0;
  uint32_t* sl = sel + r * (size_t)t;
  uint32_t* xr = xs + r * (size_t)t;
  int good = 0, distinct = 0;
  bool more = false, anydup = false;
  for (size_t c0 = 0; c0 < m; c0 += 256) {
    const size_t j = c0 + tid;
    const size_t item = r * m + j;
    const bool pred = j < m && status[item] == ST_OK;
    int total;
    const int rank = good + recw_block_rank(pred, s_w, total);
    const bool inw = pred && rank < t;
    const uint32_t id = inw ? (idx[item] & 0xFFFFu) : 0u;
    s_ids[tid] = id;
    s_in[tid] = inw ? 1 : 0;
    __syncthreads();  // (also orders the bitmap's clearing and the last chunk's bits before the reads)
    bool dup = false;
    if (inw) {
      dup = (s_bits[id >> 5] >> (id & 31)) & 1u;
      for (int k = 0; k < tid; ++k) dup = dup || (s_in[k] && s_ids[k] == id);
    }
    __syncthreads();
    if (inw && !dup) atomicOr(&s_bits[id >> 5], 1u << (id & 31));
    if (SELECT) {
      int dt;
      const int dr = distinct + recw_block_rank(inw && !dup, s_w, dt);
      if (inw && !dup) {
        sl[dr] = (uint32_t)item;
        xr[dr] = id + 1;
      }
      distinct += dt;
    } else if (inw) {
      sl[rank] = (uint32_t)item;
      xr[rank] = id + 1;
    }
    anydup = __syncthreads_or(inw && dup) || anydup;
    more = __syncthreads_or(pred && rank >= t) || more;
    good += total;
    if (good >= t && (SELECT || more)) break;
  }
  if (SELECT) {
    if (tid == 0) {  // VerifyRecovered operands: key = PubPoly.Commit() = C_0
      st_fp(rec_pk, n_rounds, r, fp_neg(ld_fp(commits, t, 0)));
      st_fp(rec_pk + FP_LIMBS * n_rounds, n_rounds, r, ld_fp(commits + FP_LIMBS * t, t, 0));
    }
    if (distinct < t) {
      if (tid < 96) out96[r * 96 + tid] = 0;
      if (tid == 0) {
        ok[r] = 0;
        st_g2a(rec_pts, n_rounds, r, g2a{fp2_zero(), fp2_zero()});
        rec_st[r] = ST_DECODE;
      }
    } else if (tid == 0) {
      ok[r] = 1;
    }
    return;
  }
  const int cnt = good < t ? good : t;
  uint8_t c;
  if (cnt < t)
    c = (want_status && cnt > 0) ? REC_EXACT : REC_FAIL;
  else if (anydup)
    c = (more || want_status) ? REC_EXACT : REC_FAIL;
  else
    c = (want_status && more) ? REC_EXACT : REC_RLC;
  if (tid == 0) {
    cls[r] = c | (more ? REC_MORE : 0);
    ok[r] = c == REC_RLC ? 1 : 0;
  }
  if (c == REC_FAIL && tid < 96) out96[r * 96 + tid] = 0;
}

// ================================================================ Lagrange
// One block per recovered round: the five slots of every (round, j) as
// k_recover_lagrange writes them, at stride t.
__global__ void __launch_bounds__(RECW_LAG_THREADS) k_recover_lagrange_wide(size_t n_rounds, int t,
                                                                            const uint8_t* __restrict__ ok,
                                                                            const uint32_t* __restrict__ xs,
                                                                            uint64_t* __restrict__ digits,
                                                                            uint64_t rlc_seed) {
  __shared__ uint32_t s_xs[RECOVER_WIDE_MAX_T];
  __shared__ fr s_segp[RECW_LAG_THREADS];
  __shared__ fr s_segx[RECW_LAG_THREADS];
  const size_t r = blockIdx.x;
  if (!ok[r]) return;  // (block-uniform)
  const int q = threadIdx.x;
  const int S = recw_lag_seg(t), nseg = recw_lag_nseg(t);
  for (int k = q; k < t; k += RECW_LAG_THREADS) s_xs[k] = xs[r * (size_t)t + k];
  __syncthreads();
  fr v[RECW_LAG_SEG];
  bool neg[RECW_LAG_SEG];
  if (q < nseg) recw_lag_step_a(s_xs, t, q, v, neg, s_segp, s_segx);
  __syncthreads();
  if (q == 0) recw_lag_step_b(s_segp, s_segx, nseg);
  __syncthreads();
  if (q >= nseg) return;
  const fr base = s_segx[q];
#pragma unroll
  for (int u = 0; u < RECW_LAG_SEG; ++u) {
    const int j = q * S + u;
    if (u >= S || j >= t) continue;
    uint32_t w[8];
    recw_lag_step_c(t, q, u, v, neg, base, w);
    const size_t g = r * (size_t)t + j;
    uint64_t* d = digits + g * RECOVER_SLOTS;
    d[0] = div_absx(w);
    d[1] = div_absx(w);
    d[2] = div_absx(w);
    d[3] = ((uint64_t)w[1] << 32) | w[0];
    d[4] = rlc_seed ? rlc_coeff(rlc_seed, g) : 0;
  }
}

// ================================================================ the MSMs
// What the two point groups give the kernels below: the group law of
// group_ops.cuh, and the loads, stores and key formats of the recovery buffers.
struct recw_g2 : G2Ops {
  using J = jac;
  using A = aff;
  static constexpr int JW = G2J_WORDS;
  static __device__ __forceinline__ bool a_is_inf(const A& a) { return fp2_is_zero(a.y); }
  static __device__ __forceinline__ A neg_if(A a, bool n) {
    a.y = fp2_cmov(a.y, fp2_neg(a.y), n);
    return a;
  }
  static __device__ __forceinline__ A ld_a(const uint32_t* b, size_t n, size_t i) { return ld_g2a(b, n, i); }
  static __device__ __forceinline__ void st_j(uint32_t* b, size_t n, size_t i, const J& p) { st_g2j(b, n, i, p); }
  // window-table entry as the Jacobian triple (X, Y in tab, Z in tabz)
  static __device__ __forceinline__ void put(uint32_t* tab, uint32_t* tabz, size_t N, size_t e, const J& p) {
    st_g2a(tab, N, e, g2a{p.x, p.y});
    st_fp(tabz, N, e, p.z.c0);
    st_fp(tabz + FP_WORDS * N, N, e, p.z.c1);
  }
  static __device__ __forceinline__ J placeholder() { return g2j{fp2_zero(), fp2_zero(), fp2_one()}; }
  // the group's share-key window table (k_pubpoly_wtable_g2) and C_0
  static __device__ __forceinline__ A ld_key(const uint32_t* wtab, size_t e) { return recover_ld_row(wtab, e); }
  // the combination A as the round's key of the pairing (k_recover_rlc_g2)
  static __device__ __forceinline__ void st_key(uint32_t* rec_key, size_t n, size_t r, const J& acc, bool ainf) {
    st_g2a(rec_key, n, r, ainf ? g2a{fp2_zero(), fp2_zero()} : g2_to_affine(acc));
  }
};
struct recw_g1 : G1Ops {
  using J = jac;
  using A = aff;
  static constexpr int JW = REC_G1J_WORDS;
  static __device__ __forceinline__ bool a_is_inf(const A& a) { return fp_is_zero(a.y); }
  static __device__ __forceinline__ A neg_if(A a, bool n) {
    a.y = fp_cmov(a.y, fp_neg(a.y), n);
    return a;
  }
  static __device__ __forceinline__ A ld_a(const uint32_t* b, size_t n, size_t i) { return rec_ld_g1a(b, n, i); }
  static __device__ __forceinline__ void st_j(uint32_t* b, size_t n, size_t i, const J& p) { rec_st_g1j(b, n, i, p); }
  static __device__ __forceinline__ void put(uint32_t* tab, uint32_t* tabz, size_t N, size_t e, const J& p) {
    rec_st_g1a(tab, N, e, g1a{p.x, p.y});
    st_fp(tabz, N, e, p.z);
  }
  static __device__ __forceinline__ J placeholder() { return g1j{fp_zero(), fp_zero(), fp_one()}; }
  // k_pubpoly_wtable's rows: x limbs then y limbs
  static __device__ __forceinline__ A ld_key(const uint32_t* wtab, size_t e) {
    const uint32_t* p = wtab + e * REC_WTAB_WORDS;
    g1a q;
#pragma unroll
    for (int l = 0; l < FP_LIMBS; ++l) {
      q.x.l[l] = p[l];
      q.y.l[l] = p[FP_LIMBS + l];
    }
    return q;
  }
  // (-x, y), the engine's pair-0 key (k_recover_rlc_g1)
  static __device__ __forceinline__ void st_key(uint32_t* rec_pk, size_t n, size_t r, const J& acc, bool ainf) {
    const g1a a = ainf ? g1a{fp_zero(), fp_zero()} : g1_to_affine(acc);
    st_fp(rec_pk, n, r, fp_neg(a.x));
    st_fp(rec_pk + FP_LIMBS * n, n, r, a.y);
  }
};

// Window tables [1..8] sig_j of the rounds [r0, r0 + nc) of a batch, as
// k_recover_tables / k_recover_tables_g1 with sel at stride t: entry
// (rl, j, m) at index (rl t + j) 8 + m of an SoA of N = nc t 8 entries.
template <class G>
__global__ void __launch_bounds__(256, 2) k_recover_tables_wide(size_t r0, size_t nc, int t,
                                                              const uint8_t* __restrict__ ok,
                                                              const uint32_t* __restrict__ sel,
                                                              const uint32_t* __restrict__ sig_pts, size_t n_items,
                                                              uint32_t* __restrict__ tab, uint32_t* __restrict__ tabz) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nc * (size_t)t) return;
  const size_t r = r0 + g / t;
  const int j = (int)(g % t);
  const size_t N = nc * (size_t)t * 8;
  if (!ok[r]) {
    const typename G::J ph = G::placeholder();
#pragma unroll 1
    for (int m = 0; m < 8; ++m) G::put(tab, tabz, N, g * 8 + m, ph);
    return;
  }
  const typename G::A q = G::ld_a(sig_pts, n_items, sel[r * (size_t)t + j]);
  typename G::J acc = G::from_aff(q);
  G::put(tab, tabz, N, g * 8, acc);
  acc = G::dbl_body(acc);
  G::put(tab, tabz, N, g * 8 + 1, acc);
#pragma unroll 1
  for (int m = 2; m < 8; ++m) {
    acc = G::add_aff_body(acc, q);
    G::put(tab, tabz, N, g * 8 + m, acc);
  }
}

// One lane's share of a Straus sum: the terms j = lig, lig + L, ... < nt over
// 17 signed radix-16 windows; entry(j, mag - 1) is [mag] point_j, affine (an
// identity entry, y = 0, is skipped).  Every addition is the generic mixed one
// (exceptional cases resolved): there is no fast path to redo.
template <class G, class E>
__device__ __forceinline__ typename G::J recw_lane_sum(int nt, int lig, int L, const uint64_t* __restrict__ d,
                                                       const E& entry) {
  typename G::J acc = G::inf();
#pragma unroll 1
  for (int w = 16; w >= 0; --w) {
    if (w < 16) {
#pragma unroll 1
      for (int s = 0; s < 4; ++s) acc = G::dbl_body(acc);
    }
#pragma unroll 1
    for (int j = lig; j < nt; j += L) {
      const int dg = win4_digit64(d[(size_t)RECOVER_SLOTS * j], w);
      const int mag = dg < 0 ? -dg : dg;
      const typename G::A e = entry(j, (mag - 1) & 7);
      const bool skip = mag == 0 || G::a_is_inf(e);
      acc = G::cmov(acc, G::add_aff_body(acc, G::neg_if(e, dg < 0)), !skip);
    }
  }
  return acc;
}

// The L lanes of every group of the block (64 threads, 64 / L groups) to the
// group's lane 0: log2 L levels, the upper half of the live lanes hands its
// sum over through LDS, complete additions (partial sums may be equal,
// opposite or the identity).  Block-uniform call.
template <class G>
__device__ __forceinline__ typename G::J recw_tree(typename G::J acc, int L, typename G::J* s_pts) {
  const int lig = threadIdx.x % L, grp = threadIdx.x / L;
  for (int h = L >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (lig >= h && lig < 2 * h) s_pts[grp * (L >> 1) + lig - h] = acc;
    __syncthreads();
    if (lig < h) acc = G::add(acc, s_pts[grp * (L >> 1) + lig]);
  }
  return acc;
}

// sum_j d_{j,i} sig_j for the slices i < `slices` of the rounds [r0, r0 + nc)
// (slice 4: the batched check's coefficients), L lanes per (round, slice),
// into part as k_recover_msm_aff / k_recover_msm_g1 leave it.
template <class G>
__global__ void __launch_bounds__(64, 2) k_recover_msm_wide(size_t n_rounds, size_t r0, size_t nc, int t, int L,
                                                           int slices, const uint8_t* __restrict__ ok,
                                                           const uint64_t* __restrict__ digits,
                                                           const uint32_t* __restrict__ tab,
                                                           uint32_t* __restrict__ part) {
  __shared__ typename G::J s_pts[32];
  const int lig = threadIdx.x % L;
  const size_t gg = (size_t)blockIdx.x * (64 / L) + threadIdx.x / L;
  const bool valid = gg < nc * (size_t)slices;
  const size_t rl = valid ? gg / slices : 0;
  const int i = valid ? (int)(gg % slices) : 0;
  const size_t r = r0 + rl;
  const bool active = valid && ok[r];
  const size_t N = nc * (size_t)t * 8;
  const size_t base = rl * (size_t)t * 8;
  typename G::J acc = recw_lane_sum<G>(active ? t : 0, lig, L, digits + r * (size_t)t * RECOVER_SLOTS + i,
                                       [&](int j, int m) { return G::ld_a(tab, N, base + (size_t)j * 8 + m); });
  acc = recw_tree<G>(acc, L, s_pts);
  if (active && lig == 0) G::st_j(part + (size_t)i * G::JW * n_rounds, n_rounds, r, acc);
}

// The batched check's combination on the key group, per REC_RLC round:
// A = C_0 + sum_j r_j Eval(i_j) over the group's share-key window table, L
// lanes per round, with k_recover_rlc_g1 / k_recover_rlc_g2's outputs (a
// candidate index >= n_group sends the round REC_EXACT).  G: the KEY group.
template <class G>
__global__ void __launch_bounds__(64, 2) k_recover_rlc_wide(size_t n_rounds, int t, int L, int n_group,
                                                           const uint32_t* __restrict__ sel,
                                                           const uint32_t* __restrict__ idx,
                                                           const uint64_t* __restrict__ digits,
                                                           const uint32_t* __restrict__ wtab,
                                                           const uint32_t* __restrict__ commits,
                                                           uint8_t* __restrict__ cls, uint8_t* __restrict__ ok,
                                                           uint32_t* __restrict__ rec_key, uint8_t* __restrict__ rec_st) {
  __shared__ typename G::J s_pts[32];
  __shared__ int s_bad[64];
  const int lig = threadIdx.x % L, grp = threadIdx.x / L;
  const size_t r = (size_t)blockIdx.x * (64 / L) + grp;
  const bool rlc = r < n_rounds && (cls[r] & 0x0F) == REC_RLC;
  const uint32_t* sl = sel + (rlc ? r : 0) * (size_t)t;
  if (lig == 0) s_bad[grp] = 0;
  __syncthreads();
  bool bad = false;
  if (rlc)
    for (int j = lig; j < t; j += L) bad = bad || idx[sl[j]] >= (uint32_t)n_group;
  if (bad) s_bad[grp] = 1;
  __syncthreads();
  const bool table_ok = !s_bad[grp];
  if (rlc && !table_ok && lig == 0) {
    cls[r] = (uint8_t)((cls[r] & REC_MORE) | REC_EXACT);
    ok[r] = 0;
    rec_st[r] = ST_DECODE;
  }
  const bool active = rlc && table_ok;
  typename G::J acc = recw_lane_sum<G>(active ? t : 0, lig, L, digits + (active ? r : 0) * (size_t)t * RECOVER_SLOTS + 4,
                                       [&](int j, int m) { return G::ld_key(wtab, (size_t)idx[sl[j]] * 8 + m); });
  acc = recw_tree<G>(acc, L, s_pts);
  if (!active || lig != 0) return;
  acc = G::add_aff_body(acc, G::ld_a(commits, t, 0));
  const bool ainf = G::is_inf(acc);
  const bool binf = rec_st[r] == ST_INFINITY;
  G::st_key(rec_key, n_rounds, r, acc, ainf);
  rec_st[r] = (ainf && binf) ? RLC_TRIVIAL : (ainf || binf) ? (uint8_t)ST_PAIRING : (uint8_t)ST_OK;
}

}  // namespace dgpu
#endif  // DG_NO_KERNELS
