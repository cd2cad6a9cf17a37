// Threshold recovery for the G1-signature schemes (bls-unchained-on-g1,
// bls-unchained-g1-rfc9380): recover.cuh with the groups swapped.  The public
// polynomial lives in G2 (commitments C_j = a_j g2, 96 bytes), a partial is
// BE16(index) || 48-byte G1 signature, and
//   VerifyPartial     e(H(msg), Eval(index)) e(-sig, g2) == 1
//   VerifyRecovered   e(H(msg), C_0) e(-sigma, g2) == 1   (the on-G1 verify
//                     path over C_0's fixed-Q line table)
//   batched check     e(H, C_0 + sum_j r_j Eval(i_j)) e(-(sigma + sum_j r_j sig_j), g2) == 1
// with the accounting of recover.cuh's header: E_j = sig_j - s_j H, the check
// holds iff sum_j (r_j + lambda_j) E_j = 0, soundness 2^-64 per failing round.
// Selection, Lagrange coefficients, round classes, gather / scatter and the
// verdict kernels are recover.cuh's, unchanged; every kernel here writes its
// recovered signature into the 96-byte round slots those kernels zero, and
// k_recover_pack48 compacts the slots to the caller's 48-byte stride.
//
// Every addition below is a generic one (exceptional cases resolved in the
// group law), so there is no fast-path / redo pair to force.
#pragma once
#include "g1sig.cuh"
#include "lines_thread.cuh"
#include "recover.cuh"

namespace dgpu {

constexpr int REC_G1J_WORDS = 3 * FP_WORDS;

__device__ __forceinline__ g1a rec_ld_g1a(const uint32_t* base, size_t n, size_t i) {
  return g1a{ld_fp(base, n, i), ld_fp(base + FP_WORDS * n, n, i)};
}
__device__ __forceinline__ void rec_st_g1a(uint32_t* base, size_t n, size_t i, const g1a& p) {
  st_fp(base, n, i, p.x);
  st_fp(base + FP_WORDS * n, n, i, p.y);
}
__device__ __forceinline__ g1j rec_ld_g1j(const uint32_t* base, size_t n, size_t i) {
  return g1j{ld_fp(base, n, i), ld_fp(base + FP_WORDS * n, n, i), ld_fp(base + 2 * FP_WORDS * n, n, i)};
}
__device__ __forceinline__ void rec_st_g1j(uint32_t* base, size_t n, size_t i, const g1j& p) {
  st_fp(base, n, i, p.x);
  st_fp(base + FP_WORDS * n, n, i, p.y);
  st_fp(base + 2 * FP_WORDS * n, n, i, p.z);
}

// ================================================================ group install
// Group commitments C_j (96-byte compressed G2, kilic's rules + subgroup
// check) -> affine SoA (stride t); rc[j] = decode code.
__global__ void k_decode_commits_g2(int t, const uint8_t* __restrict__ in96, uint32_t* __restrict__ pts,
                                    int* __restrict__ rc) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t) return;
  uint8_t buf[96];
  for (int k = 0; k < 96; ++k) buf[k] = in96[(size_t)j * 96 + k];
  g2a p{fp2_zero(), fp2_zero()};
  const int r = g2_decompress(&p, buf, true);
  st_g2a(pts, t, j, p);
  rc[j] = r;
}

// PubPoly.Eval(i) = sum_j C_j (i+1)^j in G2 by Horner (kyber share/poly.go
// (R)), affine; the identity is returned as (0, 0) (the subgroup has no point
// with y = 0, so y = 0 marks it).
__device__ g2a pubpoly_eval_g2(const uint32_t* commits, int t, uint32_t i) {
  const uint32_t x = i + 1;
  g2j acc = g2_infinity();
  for (int j = t - 1; j >= 0; --j) {
    acc = g2_mul_words(acc, &x, 1);
    acc = g2_add(acc, g2_from_affine(ld_g2a(commits, t, j)));
  }
  if (g2_is_inf(acc)) return g2a{fp2_zero(), fp2_zero()};
  return g2_to_affine(acc);
}

// Table of PubPoly.Eval(i), i < n: affine G2 SoA (stride n), the layout the
// partial decoder copies into the lines kernel's per-item keys.
__global__ void k_pubpoly_table_g2(int n, int t, const uint32_t* __restrict__ commits, uint32_t* __restrict__ table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_g2a(table, n, i, pubpoly_eval_g2(commits, t, (uint32_t)i));
}

// Window table of the share keys for the batched check: entry (i, m) =
// [m + 1] Eval(i), affine, as a G2A_WORDS row (x.c0, x.c1, y.c0, y.c1); the
// identity stores zeros.  One thread per entry, once per group.
__global__ void k_pubpoly_wtable_g2(int n, const uint32_t* __restrict__ table, uint32_t* __restrict__ wtab) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 8 * n) return;
  const int i = g >> 3;
  const uint32_t k = (uint32_t)(g & 7) + 1;
  const g2a e = ld_g2a(table, n, i);
  g2a a{fp2_zero(), fp2_zero()};
  if (!fp2_is_zero(e.y)) {
    const g2j q = g2_mul_words(g2_from_affine(e), &k, 1);
    if (!g2_is_inf(q)) a = g2_to_affine(q);
  }
  uint32_t* o = wtab + (size_t)g * G2A_WORDS;
#pragma unroll
  for (int l = 0; l < FP_LIMBS; ++l) {
    o[l] = a.x.c0.l[l];
    o[FP_LIMBS + l] = a.x.c1.l[l];
    o[2 * FP_LIMBS + l] = a.y.c0.l[l];
    o[3 * FP_LIMBS + l] = a.y.c1.l[l];
  }
}

// ================================================================ per-partial path
// Partials -> engine items, as k_decode_partials: index (BE16 of the first two
// bytes; 0xFFFFFFFF if fewer than 2), the 48-byte G1 signature after it
// decoded with the endomorphism membership test (k_decode_g1_sigs' decoder;
// any length other than 50, including 98 and one above the stride, is a
// decode error; at most 50 bytes are read), the share key Eval(index) (table
// for index < n, else evaluated here) as the item's affine G2 point.  An
// identity share key can verify nothing: ST_PAIRING.
__global__ void __launch_bounds__(256, 2) k_decode_partials_g1(size_t n_items, const uint8_t* __restrict__ partials,
                                                             size_t stride, const uint32_t* __restrict__ plen,
                                                             int n_group, int t, const uint32_t* __restrict__ table,
                                                             const uint32_t* __restrict__ commits,
                                                             uint32_t* __restrict__ sig_pts,
                                                             uint32_t* __restrict__ key_items,
                                                             uint32_t* __restrict__ idx_out,
                                                             uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const uint8_t* src = partials + i * stride;
  const uint32_t len = plen[i];
  uint32_t idx = 0xFFFFFFFFu;
  uint8_t st = ST_DECODE;
  g1a p{fp_zero(), fp_zero()};
  if (len >= 2) idx = ((uint32_t)src[0] << 8) | src[1];
  if (len == 50) {
    uint8_t buf[48];
    for (int k = 0; k < 48; ++k) buf[k] = src[2 + k];
    const int rc = g1_decompress_sig_body(&p, buf);
    st = rc == DEC_OK ? ST_OK : rc == DEC_INFINITY ? ST_INFINITY : rc == DEC_ERR_SUBGROUP ? ST_SUBGROUP : ST_DECODE;
    if (st != ST_OK) p = g1a{fp_zero(), fp_zero()};
  }
  rec_st_g1a(sig_pts, n_items, i, p);
  g2a key{fp2_zero(), fp2_zero()};
  if (st == ST_OK) {
    key = idx < (uint32_t)n_group ? ld_g2a(table, n_group, idx) : pubpoly_eval_g2(commits, t, idx);
    if (fp2_is_zero(key.y)) st = ST_PAIRING;
  }
  st_g2a(key_items, n_items, i, key);
  idx_out[i] = idx;
  status[i] = st;
}

// Affine hash points H(msg) in G1 of raw 32-byte messages under the scheme's
// DST (SoA, stride n).
__global__ void __launch_bounds__(256) k_hash_to_g1_msgs_pts(size_t n, const uint8_t* __restrict__ msgs, int g1dst,
                                                              uint32_t* __restrict__ h_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[8];
  for (int w = 0; w < 8; ++w) {
    const uint8_t* b = msgs + i * 32 + 4 * w;
    msg[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
  const g1j h = hash_to_g1(msg, g1dst != 0);
  rec_st_g1a(h_out, n, i, g1_is_inf(h) ? g1a{fp_zero(), fp_zero()} : g1_to_affine(h));
}

// The T-steps of the G1 form's two Miller loops, one thread per (item, pair)
// as k_lines_thr (same line buffer, consumed by k_eng_miller):
//   pair 0: Q = the item's G2 key (q_items, stride n: a share key, or the
//           batched check's combination), P = the hash point
//           h_pts[h_idx ? h_idx[r] : r] (stride h_stride);
//   pair 1: Q = the generator g2, P = -sig (sig_pts, stride n).
// Both signature-group points are already subgroup-checked G1 points: no
// membership test here.
__global__ void __launch_bounds__(256, DG_LINES_OCC) k_lines_thr_g1(size_t n, size_t r0, size_t cnt,
                                                                    const uint32_t* __restrict__ h_pts,
                                                                    size_t h_stride,
                                                                    const uint32_t* __restrict__ h_idx,
                                                                    const uint32_t* __restrict__ sig_pts,
                                                                    const uint32_t* __restrict__ q_items,
                                                                    uint32_t* __restrict__ lines) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;
  const int p = (int)(t & 1);
  if (i >= cnt) return;
  const size_t r = r0 + i;
  lt_q_val Qs;
  lt_pt_val P;
  if (p == 0) {
    Qs.q = ld_g2a(q_items, n, r);
    const g1a h = rec_ld_g1a(h_pts, h_stride, h_idx ? (size_t)h_idx[r] : r);
    P.nx_ = fp_neg(h.x);
    P.y_ = h.y;
  } else {
    Qs.q = g2a{C_G2_X, C_G2_Y};
    const g1a s = rec_ld_g1a(sig_pts, n, r);
    P.nx_ = fp_neg(s.x);  // -sig = (x, -y): the line takes (-x_P, y_P)
    P.y_ = fp_neg(s.y);
  }
  const size_t blk = i / ENG_ROUNDS_PER_BLOCK;
  uint32_t* base = lines + eng_blk_off(blk, ENG_LINE_STEPS, 0, (int)(i % ENG_ROUNDS_PER_BLOCK), 6 * p);
  (void)lt_pair_p(Qs, P, [&](int step, int k, const fp2& v) {
    uint2* b = reinterpret_cast<uint2*>(base + (size_t)step * FP_LIMBS * ENG_WAVE_WORDS) + k;
#pragma unroll
    for (int l = 0; l < FP_LIMBS; ++l) b[l * (ENG_WAVE_WORDS / 2)] = make_uint2(v.c0.l[l], v.c1.l[l]);
  });
}

// Synthetic partials on G1 (test/bench data tool, as k_sign_partials): item i
// is BE16(label[i]) || compress(share[sign_idx[i]] * H(msg of round i / m)),
// 50 bytes.
__global__ void __launch_bounds__(64) k_sign_partials_g1(size_t n_items, size_t m, size_t n_rounds,
                                                         const uint32_t* __restrict__ h_pts,
                                                         const uint32_t* __restrict__ sign_idx,
                                                         const uint32_t* __restrict__ label,
                                                         const scalar256* __restrict__ shares,
                                                         uint8_t* __restrict__ out50) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const g1a h = rec_ld_g1a(h_pts, n_rounds, i / m);
  const scalar256 k = shares[sign_idx[i]];
  const g1j sg = g1_mul_words(g1j{h.x, h.y, fp_one()}, k.w, 8);
  const bool inf = g1_is_inf(sg);
  uint8_t* o = out50 + i * 50;
  o[0] = (uint8_t)(label[i] >> 8);
  o[1] = (uint8_t)label[i];
  uint8_t c[48];
  g1_compress(c, inf ? g1a{fp_zero(), fp_zero()} : g1_to_affine(sg), inf);
  for (int b = 0; b < 48; ++b) o[2 + b] = c[b];
}

// ================================================================ recovery MSM
// sum_j lambda_j sig_j in G1 with k_recover_lagrange's digits: lambda = d0 +
// d1 |x| + d2 |x|^2 + d3 |x|^3 (64-bit d_i), so
//   P_i = sum_j d_{j,i} sig_j  (Straus over signed radix-16 windows, i < 4)
//   sigma = P0 + |x| (P1 + |x| (P2 + |x| P3))
// and slice 4 is the batched check's sum_j r_j sig_j.
//
// k_recover_tables_g1: one thread per (round, selected j) builds [1..8] sig_j
// (Jacobian: X, Y in tab, Z in tabz; entry (r, j, m) at index (r t + j) 8 + m
// of a G1 SoA); rounds that are not recovered write the placeholder (0, 0, 1)
// so k_g1_batch_affine's shared inversions stay sound.  The entries of a
// recovered round are never the identity (sig_j has order r).
__global__ void __launch_bounds__(256, 2) k_recover_tables_g1(size_t n_rounds, int t, const uint8_t* __restrict__ ok,
                                                            const uint32_t* __restrict__ sel,
                                                            const uint32_t* __restrict__ sig_pts, size_t n_items,
                                                            uint32_t* __restrict__ tab, uint32_t* __restrict__ tabz) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_rounds * (size_t)t) return;
  const size_t r = g / t;
  const int j = (int)(g % t);
  const size_t N = n_rounds * (size_t)t * 8;
  auto put = [&](int m, const g1j& p) {
    const size_t e = g * 8 + m;
    rec_st_g1a(tab, N, e, g1a{p.x, p.y});
    st_fp(tabz, N, e, p.z);
  };
  if (!ok[r]) {
    const g1j ph{fp_zero(), fp_zero(), fp_one()};
#pragma unroll 1
    for (int m = 0; m < 8; ++m) put(m, ph);
    return;
  }
  const g1a q = rec_ld_g1a(sig_pts, n_items, sel[r * RECOVER_MAX_T + j]);
  g1j acc{q.x, q.y, fp_one()};
  put(0, acc);
  acc = g1_dbl_body(acc);
  put(1, acc);
#pragma unroll 1
  for (int m = 2; m < 8; ++m) {
    acc = g1_add_affine_body(acc, q);
    put(m, acc);
  }
}

// `slices` threads per round (4: the digit slices of lambda; 5: also the
// batched check's coefficients): 17 signed radix-16 windows of 4 doublings
// and t mixed additions over the affine table, the same operation sequence in
// every lane (a zero digit's addition is computed and discarded).
__global__ void __launch_bounds__(256, 2) k_recover_msm_g1(size_t n_rounds, int t, const uint8_t* __restrict__ ok,
                                                         const uint64_t* __restrict__ digits,
                                                         const uint32_t* __restrict__ tab,
                                                         uint32_t* __restrict__ part, int slices) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)slices * n_rounds) return;
  const size_t r = g / slices;
  const int i = (int)(g % slices);
  if (!ok[r]) return;
  const uint64_t* d = digits + r * RECOVER_MAX_T * RECOVER_SLOTS + i;
  const size_t N = n_rounds * (size_t)t * 8;
  const size_t base = r * (size_t)t * 8;
  g1j acc = g1_infinity();
#pragma unroll 1
  for (int w = 16; w >= 0; --w) {
    if (w < 16) {
#pragma unroll 1
      for (int s = 0; s < 4; ++s) acc = g1_dbl_body(acc);
    }
#pragma unroll 1
    for (int j = 0; j < t; ++j) {
      const int dg = win4_digit64(d[RECOVER_SLOTS * j], w);
      const int mag = dg < 0 ? -dg : dg;
      g1a e = rec_ld_g1a(tab, N, base + (size_t)j * 8 + ((mag - 1) & 7));
      e.y = fp_cmov(e.y, fp_neg(e.y), dg < 0);
      acc = g1_cmov(acc, g1_add_affine_body(acc, e), mag != 0);
    }
  }
  rec_st_g1j(part + (size_t)i * REC_G1J_WORDS * n_rounds, n_rounds, r, acc);
}

// Per recovered round: sigma from the four slices, compressed into the
// round's 96-byte slot (48 bytes used); rec_pts / rec_st as k_recover_finish
// (slices = 5: B = sigma + sum_j r_j sig_j and whether B is the identity).
__global__ void __launch_bounds__(64) k_recover_finish_g1(size_t n_rounds, const uint8_t* __restrict__ ok,
                                                          const uint32_t* __restrict__ part,
                                                          uint8_t* __restrict__ out96, uint32_t* __restrict__ rec_pts,
                                                          uint8_t* __restrict__ rec_st, int slices) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rounds || !ok[r]) return;
  g1j acc = rec_ld_g1j(part + 3 * (size_t)REC_G1J_WORDS * n_rounds, n_rounds, r);
#pragma unroll 1
  for (int i = 2; i >= 0; --i)
    acc = g1_add(g1_mul_absx(acc), rec_ld_g1j(part + (size_t)i * REC_G1J_WORDS * n_rounds, n_rounds, r));
  const bool inf = g1_is_inf(acc);
  const g1a a = inf ? g1a{fp_zero(), fp_zero()} : g1_to_affine(acc);
  uint8_t c[48];
  g1_compress(c, a, inf);
  for (int k = 0; k < 48; ++k) out96[r * 96 + k] = c[k];
  for (int k = 48; k < 96; ++k) out96[r * 96 + k] = 0;
  if (slices == 5) {
    const g1j b = g1_add(acc, rec_ld_g1j(part + 4 * (size_t)REC_G1J_WORDS * n_rounds, n_rounds, r));
    const bool binf = g1_is_inf(b);
    rec_st_g1a(rec_pts, n_rounds, r, binf ? g1a{fp_zero(), fp_zero()} : g1_to_affine(b));
    rec_st[r] = binf ? (uint8_t)ST_INFINITY : (uint8_t)ST_OK;
    return;
  }
  rec_st_g1a(rec_pts, n_rounds, r, a);
  rec_st[r] = inf ? (uint8_t)ST_INFINITY : (uint8_t)ST_OK;
}

// The batched check's G2 side, per REC_RLC round, as k_recover_rlc_g1 with
// the groups swapped: A = C_0 + sum_j r_j Eval(i_j) (Straus, signed radix-16
// windows over the group's window table), stored affine as the round's pair-0
// Q for k_lines_thr_g1; rec_st combines A with B's identity flag.  A
// candidate index without a table entry (i >= n) sends the round REC_EXACT.
__global__ void __launch_bounds__(64) k_recover_rlc_g2(size_t n_rounds, int t, int n_group,
                                                       const uint32_t* __restrict__ sel,
                                                       const uint32_t* __restrict__ idx,
                                                       const uint64_t* __restrict__ digits,
                                                       const uint32_t* __restrict__ wtab,
                                                       const uint32_t* __restrict__ commits, uint8_t* __restrict__ cls,
                                                       uint8_t* __restrict__ ok, uint32_t* __restrict__ rec_key,
                                                       uint8_t* __restrict__ rec_st) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rounds || (cls[r] & 0x0F) != REC_RLC) return;
  const uint32_t* sl = sel + r * RECOVER_MAX_T;
  const uint64_t* d = digits + r * RECOVER_MAX_T * RECOVER_SLOTS + 4;
  bool table_ok = true;
  for (int j = 0; j < t; ++j) table_ok = table_ok && idx[sl[j]] < (uint32_t)n_group;
  if (!table_ok) {
    cls[r] = (uint8_t)((cls[r] & REC_MORE) | REC_EXACT);
    ok[r] = 0;
    rec_st[r] = ST_DECODE;
    return;
  }
  g2j acc = g2_infinity();
#pragma unroll 1
  for (int w = 16; w >= 0; --w) {
    if (w < 16) {
#pragma unroll 1
      for (int s = 0; s < 4; ++s) acc = g2_dbl(acc);
    }
#pragma unroll 1
    for (int j = 0; j < t; ++j) {
      const int dg = win4_digit64(d[RECOVER_SLOTS * j], w);
      const int mag = dg < 0 ? -dg : dg;
      g2a q = recover_ld_row(wtab, (size_t)idx[sl[j]] * 8 + ((mag - 1) & 7));
      const bool qinf = fp2_is_zero(q.y);
      q.y = fp2_cmov(q.y, fp2_neg(q.y), dg < 0);
      acc = g2_cmov(acc, g2_add_affine(acc, q), mag != 0 && !qinf);
    }
  }
  acc = g2_add_affine(acc, ld_g2a(commits, t, 0));
  const bool ainf = g2_is_inf(acc);
  const bool binf = rec_st[r] == ST_INFINITY;
  st_g2a(rec_key, n_rounds, r, ainf ? g2a{fp2_zero(), fp2_zero()} : g2_to_affine(acc));
  rec_st[r] = (ainf && binf) ? RLC_TRIVIAL : (ainf || binf) ? (uint8_t)ST_PAIRING : (uint8_t)ST_OK;
}

// The 96-byte round slots -> the caller's 48-byte stride (zero unless recovered).
__global__ void __launch_bounds__(256) k_recover_pack48(size_t n_rounds, const uint8_t* __restrict__ slots96,
                                                        const uint8_t* __restrict__ ok, uint8_t* __restrict__ out48) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_rounds * 48) return;
  const size_t r = g / 48, k = g % 48;
  out48[g] = ok[r] ? slots96[r * 96 + k] : (uint8_t)0;
}

}  // namespace dgpu
