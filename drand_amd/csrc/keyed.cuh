// Verification under a key per record (dgpu_verify_keyed[_device]; include/
// drand_gpu.h): the batch form of bls.Verify(key[key_idx[i]], msg_i, sig_i), the
// loop of Identity.ValidSignature / Group.UnsignedIdentities (key/keys.go:52-63,
// key/group.go:474-482) and of a validator that follows several chains.
//
// The call's key table is decoded on the device by the commitment decoders
// (k_decode_commits, k_decode_commits_g2: dgpu_decode_pubkey's rules, subgroup
// check included), one decode code per table entry.  The gather below turns
// the table into the per-item keys the lines kernels already read
// (pairing_job::pk_items / g1form_keys) and gives every record that names a
// rejected key, or an index outside the table, the final status ST_KEY.  The
// host never reads the decode codes: the device form stays asynchronous.
//
// RLC mode (n >= DGPU_RLC_MIN): a batch under K keys splits into K independent
// random linear combinations, one 2-pairing check per key:
//   leaves   P_i = [a_i] H_i + [b_i] endo(H_i), S_i likewise from sig_i, with
//            (a_i, b_i) the halves of rlc_coeff(seed, i); H_i is the full,
//            cofactor-cleared hash point, so no node needs a second clearing;
//            records whose status is already final contribute nothing
//   groups   the undecided records listed by key: count, scan, scatter
//            (keyed_groups.h)
//   sums     per key, P_g and S_g: equal list ranges per thread and a fix-up
//            pass (keyed_groups.h), Jacobian, with the complete addition
//   nodes    one candidate per non-empty key, compacted to the front, with
//            k_rlc_prep's status rule and the key itself as the item's key
//   fallback every undecided record of a failing key is listed for an exact
//            per-record pairing (no bisection inside a key's group)
// Soundness: signatures are subgroup-checked by their decoders before any
// combination (as rlc_points_locked documents) and table keys at decode.
// dgpu_verify_partials is the second front end of the same core: the group id
// is the share index, the key the share key PubPoly.Eval(index) the partial
// decoder left per item, and the hash point is the round's, read through h_idx.
// The fix-up runs a wave per group: a group of c records has c / R pieces,
// which one thread per group would join in one serial chain.
#pragma once
#include "kernels.cuh"
#include "keyed_groups.h"
#include "recover.cuh"
#include "recover_g1.cuh"
#include "rlc_msm.cuh"

namespace dgpu {

// The record's key is unusable (DGPU_REASON_KEY): it outranks the record's own
// signature status, as the reference decodes the key before the signature.
constexpr uint8_t ST_KEY = 5;
constexpr size_t KEYED_MAX_KEYS = 65536;

#ifndef DG_NO_KERNELS

// Item i's key = table entry key_idx[i].  G2KEY = false: the table holds affine
// G1 points (x, y), SoA with stride n_keys; keys_out the engine's (-x, y), SoA
// with stride n.  G2KEY = true: affine G2 points on both sides.  A rejected
// entry (rc != DEC_OK: undecodable, outside the subgroup, the identity) or an
// index >= n_keys reads nothing from the table, stores a zero key and sets
// status[i] = ST_KEY over whatever the signature decode left there.
template <bool G2KEY>
__global__ void __launch_bounds__(256) k_keyed_gather(size_t n, uint32_t n_keys, const uint32_t* __restrict__ key_idx,
                                                      const uint32_t* __restrict__ table, const int* __restrict__ rc,
                                                      uint32_t* __restrict__ keys_out, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key_idx[i];
  const bool good = k < n_keys && rc[k] == DEC_OK;
  if constexpr (G2KEY) {
    st_g2a(keys_out, n, i, good ? ld_g2a(table, n_keys, k) : g2a{fp2_zero(), fp2_zero()});
  } else {
    fp nx = fp_zero(), y = fp_zero();
    if (good) {
      nx = fp_neg(ld_fp(table, n_keys, k));
      y = ld_fp(table + (size_t)FP_LIMBS * n_keys, n_keys, k);
    }
    st_fp(keys_out, n, i, nx);
    st_fp(keys_out + (size_t)FP_LIMBS * n, n, i, y);
  }
  if (!good) status[i] = ST_KEY;
}

// ---------------------------------------------------------------- RLC mode
// Leaves, 2n threads (j < n: P_j, else S_{j-n}) as k_rlc_leaves, the hash
// point read through h_idx (null: i) from an array of stride h_stride.
template <class Gr>
__global__ void __launch_bounds__(256, 2) k_keyed_leaves(size_t n, uint64_t seed, const uint32_t* __restrict__ h_pts,
                                                         size_t h_stride, const uint32_t* __restrict__ h_idx,
                                                         const uint32_t* __restrict__ sig_pts,
                                                         const uint8_t* __restrict__ status,
                                                         uint32_t* __restrict__ p_out, uint32_t* __restrict__ s_out) {
  using M = GrMem<Gr>;
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * n) return;
  const bool sig = j >= n;
  const size_t i = sig ? j - n : j;
  typename Gr::jac acc = Gr::inf();
  if (status[i] == ST_OK) {
    const typename Gr::aff q = sig ? M::ld_aff(sig_pts, n, i) : M::ld_aff(h_pts, h_stride, h_idx ? (size_t)h_idx[i] : i);
    if (!Gr::aff_is_zero(q)) {
      const uint64_t z = rlc_coeff(seed, i);
      if constexpr (std::is_same<Gr, G2Ops>::value)
        acc = g2_mul2_win4_affine(q, (uint32_t)z, (uint32_t)(z >> 32));
      else
        acc = mul2_win4_affine<Gr>(q, (uint32_t)z, (uint32_t)(z >> 32));
    }
  }
  M::st_jac(sig ? s_out : p_out, n, i, acc);
}

// counts[g] = undecided records (status ST_OK) of group g = gid[i] (< n_groups:
// a keyed record outside the table is ST_KEY already; a partial whose share
// index is above the group's table takes no part and goes to the exact check).
__global__ void __launch_bounds__(256) k_keyed_count(size_t n, uint32_t n_groups, const uint32_t* __restrict__ gid,
                                                     const uint8_t* __restrict__ status, uint32_t* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != ST_OK) return;
  const uint32_t g = gid[i];
  if (g < n_groups) atomicAdd(counts + g, 1u);
}

// One block: exclusive prefix sums of the counts -> offsets (and the scatter's
// cursors), and of the non-empty flags -> cpos (a non-empty group's candidate
// slot); totals[0] = listed records, totals[1] = non-empty groups.  Thread t
// covers keyed_scan_per(n_groups) consecutive groups.
__global__ void __launch_bounds__(KEYED_SCAN_THREADS) k_keyed_scan(uint32_t n_groups, const uint32_t* __restrict__ counts,
                                                                   uint32_t* __restrict__ offsets,
                                                                   uint32_t* __restrict__ cursor,
                                                                   uint32_t* __restrict__ cpos,
                                                                   uint32_t* __restrict__ totals) {
  __shared__ uint32_t part[KEYED_SCAN_THREADS], used[KEYED_SCAN_THREADS];
  const int t = threadIdx.x;
  const size_t per = keyed_scan_per(n_groups);
  const size_t g0 = (size_t)t * per, g1 = g0 + per < n_groups ? g0 + per : n_groups;
  uint32_t sum = 0, ne = 0;
  for (size_t g = g0; g < g1; ++g) sum += counts[g], ne += counts[g] != 0;
  part[t] = sum, used[t] = ne;
  __syncthreads();
  for (int off = 1; off < KEYED_SCAN_THREADS; off <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = t >= off ? part[t - off] : 0u, w = t >= off ? used[t - off] : 0u;
    __syncthreads();
    part[t] += v, used[t] += w;
    __syncthreads();
  }
  uint32_t run = part[t] - sum, slot = used[t] - ne;
  for (size_t g = g0; g < g1; ++g) {
    offsets[g] = run, cursor[g] = run, cpos[g] = slot;
    run += counts[g], slot += counts[g] != 0;
  }
  if (t == KEYED_SCAN_THREADS - 1) totals[0] = part[t], totals[1] = used[t];
}

// list[pos] = i and lkey[pos] = its group, pos from the group's cursor.
__global__ void __launch_bounds__(256) k_keyed_scatter(size_t n, uint32_t n_groups, const uint32_t* __restrict__ gid,
                                                       const uint8_t* __restrict__ status, uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ list, uint32_t* __restrict__ lkey) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != ST_OK) return;
  const uint32_t g = gid[i];
  if (g >= n_groups) return;
  const uint32_t pos = atomicAdd(cursor + g, 1u);
  list[pos] = (uint32_t)i;
  lkey[pos] = g;
}

// The sums of range t (keyed_groups.h), 2T threads: the first T on the P
// leaves, the rest on the S leaves.  sums: [P | S], each a Jacobian SoA of
// stride n_groups; part: [P | S], each [A | B] of stride 2T.  Complete
// additions (a group may hold one record twice, or a record and its negative).
template <class Gr>
__global__ void __launch_bounds__(256) k_keyed_sums(size_t T, size_t R, const uint32_t* __restrict__ totals,
                                                    uint32_t n_groups, const uint32_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ counts,
                                                    const uint32_t* __restrict__ list, const uint32_t* __restrict__ lkey,
                                                    size_t n, const uint32_t* __restrict__ p_leaf,
                                                    const uint32_t* __restrict__ s_leaf, uint32_t* __restrict__ sums,
                                                    uint32_t* __restrict__ part) {
  using M = GrMem<Gr>;
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= 2 * T) return;
  const bool sig = id >= T;
  const size_t t = sig ? id - T : id;
  const size_t L = totals[0];
  const size_t p0 = t * R;
  if (p0 >= L) return;
  const size_t p1 = p0 + R < L ? p0 + R : L;
  const uint32_t* leaf = sig ? s_leaf : p_leaf;
  uint32_t* const gsum = sums + (sig ? (size_t)n_groups * M::JAC : 0);
  uint32_t* const gpart = part + (sig ? 2 * T * M::JAC : 0);
  auto emit = [&](uint32_t g, size_t s, size_t e, const typename Gr::jac& acc) {
    const int kind = keyed_run_kind(s, e, offsets[g], counts[g]);
    if (kind == KEYED_RUN_WHOLE) M::st_jac(gsum, n_groups, g, acc);
    else M::st_jac(gpart, 2 * T, kind == KEYED_RUN_HEAD ? t : T + t, acc);
  };
  uint32_t g = lkey[p0];
  size_t s = p0;
  typename Gr::jac acc = Gr::inf();
#pragma unroll 1
  for (size_t p = p0; p < p1; ++p) {
    const uint32_t k = lkey[p];
    if (k != g) {
      emit(g, s, p, acc);
      g = k, s = p;
      acc = Gr::inf();
    }
    acc = Gr::add(acc, M::ld_jac(leaf, n, list[p]));
  }
  emit(g, s, p1, acc);
}

// One wave per (group, point set), 2 n_groups blocks (P, then S): an empty
// group's sum is the identity; a group that spans ranges t0 < t1 is
// B[t0] + A[t0 + 1] + ... + A[t1].  A group of c records has c / R such
// pieces, so one thread per group would be a serial chain as long as the
// largest group: lane l adds A[t0 + 1 + l], A[t0 + 1 + l + 64], ..., puts its
// sum back into its first slot (no other lane reads it) and the 64 slots are
// halved six times.  The pieces are consumed: nothing reads `part` afterwards.
template <class Gr>
__global__ void __launch_bounds__(64) k_keyed_fixup(size_t T, size_t R, uint32_t n_groups,
                                                    const uint32_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ counts, uint32_t* part,
                                                    uint32_t* __restrict__ sums) {
  using M = GrMem<Gr>;
  const size_t id = blockIdx.x;
  if (id >= 2 * (size_t)n_groups) return;
  const size_t lane = threadIdx.x;
  const bool sig = id >= n_groups;
  const size_t g = sig ? id - n_groups : id;
  uint32_t* const gsum = sums + (sig ? (size_t)n_groups * M::JAC : 0);
  uint32_t* const gpart = part + (sig ? 2 * T * M::JAC : 0);
  const size_t c = counts[g];  // (every exit below is taken by the whole block)
  if (c == 0) {
    if (lane == 0) M::st_jac(gsum, n_groups, g, Gr::inf());
    return;
  }
  size_t t0, t1;
  if (!keyed_group_split(offsets[g], c, R, &t0, &t1)) return;
  const size_t m = t1 - t0, a0 = t0 + 1;  // the pieces A[a0 .. a0 + m)
  if (lane < m) {
    typename Gr::jac acc = M::ld_jac(gpart, 2 * T, a0 + lane);
#pragma unroll 1
    for (size_t k = lane + 64; k < m; k += 64) acc = Gr::add(acc, M::ld_jac(gpart, 2 * T, a0 + k));
    M::st_jac(gpart, 2 * T, a0 + lane, acc);
  }
  __syncthreads();
#pragma unroll 1
  for (size_t stride = 32; stride >= 1; stride >>= 1) {
    if (lane < stride && lane + stride < m)
      M::st_jac(gpart, 2 * T, a0 + lane,
                Gr::add(M::ld_jac(gpart, 2 * T, a0 + lane), M::ld_jac(gpart, 2 * T, a0 + lane + stride)));
    __syncthreads();
  }
  if (lane == 0) M::st_jac(gsum, n_groups, g, Gr::add(M::ld_jac(gpart, 2 * T, T + t0), M::ld_jac(gpart, 2 * T, a0)));
}

// One candidate per non-empty group g, in slot c = cpos[g] of m slots: affine
// P_g and S_g, k_rlc_prep's status rule (no cofactor step: the leaves carry
// the full hash), and the group's key copied from the per-item key of the
// group's first listed record (kw words, SoA with stride n -> stride m: every
// record of a group carries the same key, in the layout the engine reads).
// The slots past the non-empty groups keep what the host put there
// (RLC_TRIVIAL, zero points).
template <class Gr>
__global__ void __launch_bounds__(64) k_keyed_prep(uint32_t n_groups, size_t m, const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ cpos,
                                                   const uint32_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ list, const uint32_t* __restrict__ sums,
                                                   size_t n, const uint32_t* __restrict__ item_keys, int kw,
                                                   uint32_t* __restrict__ h_out, uint32_t* __restrict__ s_out,
                                                   uint32_t* __restrict__ keys_out, uint8_t* __restrict__ st) {
  using M = GrMem<Gr>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups || counts[g] == 0) return;
  const size_t c = cpos[g];
  if (c >= m) return;
  const typename Gr::jac P = M::ld_jac(sums, n_groups, g);
  const typename Gr::jac S = M::ld_jac(sums + (size_t)n_groups * M::JAC, n_groups, g);
  const bool pi = Gr::is_inf(P), si = Gr::is_inf(S);
  M::st_aff(h_out, m, c, pi ? Gr::aff_zero() : Gr::to_aff(P));
  M::st_aff(s_out, m, c, si ? Gr::aff_zero() : Gr::to_aff(S));
  const size_t i = list[offsets[g]];
  for (int w = 0; w < kw; ++w) keys_out[(size_t)w * m + c] = item_keys[(size_t)w * n + i];
  st[c] = (pi && si) ? RLC_TRIVIAL : (pi || si) ? (uint8_t)ST_PAIRING : (uint8_t)ST_OK;
}

// The undecided records of every failing group, and those whose group id lies
// outside the grouped range (a partial whose share index is above the group's
// table: no combination, straight to the exact check), listed for the exact
// check (order irrelevant); nfail[0] counts them.
__global__ void __launch_bounds__(256) k_keyed_list_failing(size_t n, uint32_t n_groups, const uint32_t* __restrict__ gid,
                                                            const uint8_t* __restrict__ status,
                                                            const uint32_t* __restrict__ cpos,
                                                            const uint8_t* __restrict__ cand_st,
                                                            uint32_t* __restrict__ flist, uint32_t* __restrict__ nfail) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != ST_OK) return;
  const uint32_t g = gid[i];
  bool exact = g >= n_groups;
  if (!exact) {
    const uint8_t cs = cand_st[cpos[g]];
    exact = cs != ST_OK && cs != RLC_TRIVIAL;
  }
  if (exact) flist[atomicAdd(nfail, 1u)] = (uint32_t)i;
}

// The listed records as a compact batch of m items: hash point (through
// h_idx), signature point and key (kw words per key, SoA with stride n ->
// stride m), status ST_OK.
__global__ void __launch_bounds__(256) k_keyed_compact(size_t m, const uint32_t* __restrict__ flist, size_t n,
                                                       const uint32_t* __restrict__ h_pts, size_t h_stride,
                                                       const uint32_t* __restrict__ h_idx,
                                                       const uint32_t* __restrict__ sig_pts, int aw,
                                                       const uint32_t* __restrict__ keys, int kw,
                                                       uint32_t* __restrict__ h_out, uint32_t* __restrict__ s_out,
                                                       uint32_t* __restrict__ k_out, uint8_t* __restrict__ st_out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const size_t i = flist[k], hi = h_idx ? (size_t)h_idx[i] : i;
  for (int w = 0; w < aw; ++w) {
    h_out[(size_t)w * m + k] = h_pts[(size_t)w * h_stride + hi];
    s_out[(size_t)w * m + k] = sig_pts[(size_t)w * n + i];
  }
  for (int w = 0; w < kw; ++w) k_out[(size_t)w * m + k] = keys[(size_t)w * n + i];
  st_out[k] = ST_OK;
}

// The exact check's verdicts back to the records.
__global__ void __launch_bounds__(256) k_keyed_scatter_verdicts(size_t m, const uint32_t* __restrict__ flist,
                                                                const uint8_t* __restrict__ st_in,
                                                                uint8_t* __restrict__ status) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m && st_in[k] != ST_OK) status[flist[k]] = st_in[k];
}

#endif  // DG_NO_KERNELS

}  // namespace dgpu
