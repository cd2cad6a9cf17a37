// Miller-loop arithmetic with one Fp2 coefficient per lane (DESIGN.md section
// 2b, "six lanes").  Six lanes cooperate on one item: lane m owns coefficient
// f_m of f = sum f_m w^m (w^6 = xi = 1 + u), ten items per wave.  A lane that
// owns both halves of its coefficient can form an Fp2 product by Karatsuba,
// 3 Fp products instead of the 4 of the 12-lane model (engine.cuh), without
// exchanging unreduced accumulators between lanes.
//
// Item state in LDS, 36 slots of 14 words (2,016 bytes):
//   slot 4m + 0..3   f_m as (re, im, re - im + 8p, re + im); the last two are
//                    xi f_m, written by the owning lane with the coefficient
//   slot 24 + 6L + e line L's coefficients (l0, l2, l3) as (re, im) pairs
// Every stored value has normalized limbs (< 2^28 below the top limb).
//
// One output sum_t a_t b_t over Fp2 (a_t = a0 + a1 u, b_t = b0 + b1 u):
//   U = sum a0 b0, S = sum a1 b1                     (27 product columns each)
//   re = redc(U - S + p R)                           (columns signed)
//   W = sum (a0 + a1)(b0 + b1), im = redc(W - (U + S))
// The operand sums are limb-wise, so column k of W is column k of
// U + S + (a0 b1 + a1 b0) exactly: W - (U + S) is non-negative column by
// column, and the 64-bit wrap-around of an intermediate column is harmless.
// U - S can be negative in a column: its reduction carries in signed
// arithmetic and adds p R (p in columns 14..27), which makes the total
// non-negative for |U - S| < p R.  No multiple of p that dominates S column
// by column is needed.
//
// Column bounds (limbs: stored values < 2^28, a doubled b < 2^29; a column
// has at most 13 full-size products, the top limbs are < 2^21):
//   line product, 3 terms:  |U - S| < 3 * 13 * 2^56 < 2^61.3
//                           W - (U + S) < 6 * 13 * 2^56 < 2^62.3
//   squaring, 3 doubled terms and the plain square f_i^2 = (d s, 2 re im):
//                           |U - S| < 7 * 13 * 2^56 < 2^62.6   (< 2^63, signed)
//                           W - (U + S) < 14 * 13 * 2^56 < 2^63.6 (< 2^64 - 2^60)
// Values: the sums are below 14 * (10.3p)(4.5p) < 650 p^2 = 0.26 p R, so both
// outputs are below 2.3p with normalized limbs; re - im + 8p < 10.3p and
// re + im < 4.6p keep FP_SUBK's precondition (subtrahend < 7.99p).
#pragma once
#include "engine.cuh"
#include "engine_layout.cuh"

namespace dgpu {

constexpr int M6_LANES = 6;            // lanes per item
constexpr int M6_ITEMS_PER_WAVE = 10;  // lanes 60..63 repeat lanes 54..57
constexpr int M6_BLOCKS_PER_WAVE = M6_ITEMS_PER_WAVE / ENG_ROUNDS_PER_BLOCK;
constexpr int M6_COEF_WORDS = 4 * ENG_SLOT_WORDS;
constexpr int M6_L1 = 24, M6_L2 = 30, M6_SLOTS = 36;
constexpr int M6_ITEM_WORDS = M6_SLOTS * ENG_SLOT_WORDS;
static_assert(M6_ITEMS_PER_WAVE * M6_LANES <= 64 && M6_ITEMS_PER_WAVE % ENG_ROUNDS_PER_BLOCK == 0, "whole blocks per wave");
// N1 = Norm(f) stays on the 12-lane program: its last ops (M_XIF, M_NRM, M_XIN2, M_T012, M_XIT, M_D, M_N1), which
// read f's slots and the constants alone (miller6_kernels.cuh k_eng_miller_tail)
constexpr int ENG_MILLER_TAIL_OPS = 7;

// ---------------------------------------------------------------- addressing
// Lane `lane` of wave `wave`: item gi = lane / 6 of the wave, coefficient m.
// Item 10 wave + gi is round g = gi % 5 of block 2 wave + gi / 5.  Lane m
// moves words 2m and 2m + 1 of its item's 12-word rows, which are adjacent and
// 8-byte aligned (eng_blk_off is even for even e): in a line row they are one
// Fp2 line coefficient (line 1's l0, l2, l3, then line 2's), in the f plane
// (re, im) of f_m.  With an odd number of blocks the last wave's second half
// reads the last block again and writes nothing, so every access stays inside
// eng_blk_words(eng_blocks(cnt), .).
struct m6_lane {
  int gi, m, g;
  size_t blk;
  bool valid;
};
DG_FN m6_lane m6_lane_id(size_t cnt, size_t wave, int lane) {
  m6_lane L;
  L.gi = lane < M6_ITEMS_PER_WAVE * M6_LANES ? lane / M6_LANES : M6_ITEMS_PER_WAVE - 1;
  L.m = lane < M6_ITEMS_PER_WAVE * M6_LANES ? lane % M6_LANES : lane - M6_ITEMS_PER_WAVE * M6_LANES;
  L.g = L.gi % ENG_ROUNDS_PER_BLOCK;
  L.blk = wave * M6_BLOCKS_PER_WAVE + L.gi / ENG_ROUNDS_PER_BLOCK;
  L.valid = L.blk * ENG_ROUNDS_PER_BLOCK + L.g < cnt;
  const size_t nblk = eng_blocks(cnt);
  if (L.blk >= nblk) L.blk = nblk - 1;
  return L;
}
// word offset of limb 0 of the lane's two words; limb l is l * ENG_WAVE_WORDS further
DG_FN size_t m6_line_off(const m6_lane& L, int step) { return eng_blk_off(L.blk, ENG_LINE_STEPS, step, L.g, 2 * L.m); }
DG_FN size_t m6_f_off(const m6_lane& L) { return eng_blk_off(L.blk, ENG_F_PLANES, 0, L.g, 2 * L.m); }

// The loop's schedule over the ENG_LINE_STEPS line steps (each is two line
// products): the 63 doubling steps follow bits 62..0 of |x|, every one but
// the first opens with the squaring, and a set bit adds an addition step.
constexpr uint64_t M6_LOOP_X = 0xD201000000010000ull;
struct m6_sched {
  int j = 62;
  bool second = false;  // the addition step of a set bit
};
DG_FN bool m6_sched_sqr(const m6_sched& s) { return !s.second && s.j != 62; }
DG_FN void m6_sched_next(m6_sched& s) {
  if (!s.second && ((M6_LOOP_X >> s.j) & 1u)) {
    s.second = true;
  } else {
    s.second = false;
    --s.j;
  }
}

// One Fp2 product term: a = (a0, a1) and b = (b0, b1) in consecutive slots;
// b is doubled when sh == 1.
struct m6_term {
  const uint32_t* a;
  const uint32_t* b;
  uint32_t sh;
};

template <bool FIRST>
DG_FN void m6_mac(uint64_t* col, const fp& a, const fp& b) {
#pragma unroll
  for (int i = 0; i < FP_LIMBS; ++i) {
#pragma unroll
    for (int j = 0; j < FP_LIMBS; ++j) {
      const uint64_t p = (uint64_t)a.l[i] * b.l[j];
      col[i + j] = (FIRST && (i == 0 || j == FP_LIMBS - 1)) ? p : col[i + j] + p;
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // one term's products complete before the next term's operands are loaded
  // (engine.cuh eng_sub_c: otherwise every term's operands stay live)
#pragma unroll
  for (int q = 0; q < 2 * FP_LIMBS - 1; ++q) asm volatile("" : "+v"(col[q]));
#endif
}

DG_FN fp m6_shl(const fp& a, uint32_t sh) {
  fp r;
#pragma unroll
  for (int i = 0; i < FP_LIMBS; ++i) r.l[i] = a.l[i] << sh;
  return r;
}

// Montgomery reduction of signed columns t[k] (|t[k]| < 2^63 - 2^60, two's
// complement) with p R added: (T + p R) / R mod p for |T| < p R, normalized
// limbs, < T / R + 2p.  fp_redc_cols with an arithmetic carry shift.
DG_FN fp m6_redc_signed(const uint64_t* t) {
  fp r;
  uint32_t m[FP_LIMBS];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < FP_LIMBS; ++k) {
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (uint64_t)m[i] * FP_P[k - i];
    acc += t[k];
    m[k] = ((uint32_t)acc * FP_PINV) & FP_MASK;
    acc += (uint64_t)m[k] * FP_P[0];
    acc = (uint64_t)((int64_t)acc >> FP_BITS);
  }
#pragma unroll
  for (int k = FP_LIMBS; k < 2 * FP_LIMBS; ++k) {
#pragma unroll
    for (int i = k - FP_LIMBS + 1; i < FP_LIMBS; ++i) acc += (uint64_t)m[i] * FP_P[k - i];
    acc += FP_P[k - FP_LIMBS];
    if (k < 2 * FP_LIMBS - 1) {
      acc += t[k];
      r.l[k - FP_LIMBS] = (uint32_t)acc & FP_MASK;
      acc = (uint64_t)((int64_t)acc >> FP_BITS);
    } else {
      r.l[k - FP_LIMBS] = (uint32_t)acc;
    }
  }
  return r;
}

// (re, im) = sum of NT Fp2 products, plus (SQ, on lanes with sq != nullptr)
// the plain square of the coefficient at sq: re += (re - im)(re + im),
// im += 2 re im.
template <int NT, bool SQ>
DG_FN void m6_fp2_sum(const m6_term* tm, const uint32_t* sq, fp& re, fp& im) {
  uint64_t U[2 * FP_LIMBS - 1], S[2 * FP_LIMBS - 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const fp a0 = eng_ld(tm[t].a);
    const fp b0 = m6_shl(eng_ld(tm[t].b), SQ ? tm[t].sh : 0u);
    if (t == 0) m6_mac<true>(U, a0, b0);
    else m6_mac<false>(U, a0, b0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const fp a1 = eng_ld(tm[t].a + ENG_SLOT_WORDS);
    const fp b1 = m6_shl(eng_ld(tm[t].b + ENG_SLOT_WORDS), SQ ? tm[t].sh : 0u);
    if (t == 0) m6_mac<true>(S, a1, b1);
    else m6_mac<false>(S, a1, b1);
  }
#pragma unroll
  for (int k = 0; k < 2 * FP_LIMBS - 1; ++k) {
    const uint64_t u = U[k], s = S[k];
    U[k] = u - s;
    S[k] = u + s;
  }
  if constexpr (SQ) {
    if (sq) m6_mac<false>(U, eng_ld(sq + 2 * ENG_SLOT_WORDS), eng_ld(sq + 3 * ENG_SLOT_WORDS));
  }
  re = m6_redc_signed(U);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const fp as = fp_add_lz(eng_ld(tm[t].a), eng_ld(tm[t].a + ENG_SLOT_WORDS));
    const fp bs = m6_shl(fp_add_lz(eng_ld(tm[t].b), eng_ld(tm[t].b + ENG_SLOT_WORDS)), SQ ? tm[t].sh : 0u);
    if (t == 0) m6_mac<true>(U, as, bs);
    else m6_mac<false>(U, as, bs);
  }
  if constexpr (SQ) {
    if (sq) m6_mac<false>(U, eng_ld(sq), m6_shl(eng_ld(sq + ENG_SLOT_WORDS), 1u));
  }
  uint64_t W[2 * FP_LIMBS];
#pragma unroll
  for (int k = 0; k < 2 * FP_LIMBS - 1; ++k) W[k] = U[k] - S[k];
  W[2 * FP_LIMBS - 1] = 0;
  im = fp_redc_cols(W);
}

// The owning lane's write: the coefficient and xi times it.
DG_FN void m6_store(uint32_t* it, int m, const fp& re, const fp& im) {
  uint32_t* p = it + m * M6_COEF_WORDS;
  eng_st(p, re);
  eng_st(p + ENG_SLOT_WORDS, im);
  eng_st(p + 2 * ENG_SLOT_WORDS, eng_cyc_sum(re, im, true));
  eng_st(p + 3 * ENG_SLOT_WORDS, eng_cyc_sum(re, im, false));
}

// Lane m's coefficient of f * (l0 + l2 w^2 + l3 w^3), the line at slot
// `line` (M6_L1 or M6_L2): f_m l0 + f_(m-2) l2 + f_(m-3) l3, where an index
// below 0 wraps to m + 6 and takes xi f.
DG_FN void m6_line_mul(const uint32_t* it, int m, int line, fp& re, fp& im) {
  m6_term tm[3];
  const int sh[3] = {0, 2, 3};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const bool wrap = m < sh[t];
    const int src = m - sh[t] + (wrap ? 6 : 0);
    tm[t].a = it + src * M6_COEF_WORDS + (wrap ? 2 * ENG_SLOT_WORDS : 0);
    tm[t].b = it + (line + 2 * t) * ENG_SLOT_WORDS;
    tm[t].sh = 0;
  }
  m6_fp2_sum<3, false>(tm, nullptr, re, im);
}

// Lane m's coefficient of f^2 in the direct form: the pairs i <= j with
// i + j = m or m + 6 (the latter with xi f_j).  Each lane has three Fp2
// products (cross terms doubled; on even lanes the third is the wrapped
// square f_i (xi f_i), not doubled), and even lanes add the plain square
// f_(m/2)^2: 11 Fp products on even lanes, 9 on odd ones.
// Per term: i | j << 3 | wrap << 6 | doubled << 7; bits 24..26 the plain
// square's index, bit 27 set when the lane has one.
DG_FN uint32_t m6_sqr_word(int m) {
#define M6_T(i, j, w, d) ((uint32_t)((i) | (j) << 3 | (w) << 6 | (d) << 7))
  constexpr uint32_t W0 = M6_T(1, 5, 1, 1) | M6_T(2, 4, 1, 1) << 8 | M6_T(3, 3, 1, 0) << 16 | 0u << 24 | 1u << 27;
  constexpr uint32_t W1 = M6_T(0, 1, 0, 1) | M6_T(2, 5, 1, 1) << 8 | M6_T(3, 4, 1, 1) << 16;
  constexpr uint32_t W2 = M6_T(0, 2, 0, 1) | M6_T(3, 5, 1, 1) << 8 | M6_T(4, 4, 1, 0) << 16 | 1u << 24 | 1u << 27;
  constexpr uint32_t W3 = M6_T(0, 3, 0, 1) | M6_T(1, 2, 0, 1) << 8 | M6_T(4, 5, 1, 1) << 16;
  constexpr uint32_t W4 = M6_T(0, 4, 0, 1) | M6_T(1, 3, 0, 1) << 8 | M6_T(5, 5, 1, 0) << 16 | 2u << 24 | 1u << 27;
  constexpr uint32_t W5 = M6_T(0, 5, 0, 1) | M6_T(1, 4, 0, 1) << 8 | M6_T(2, 3, 0, 1) << 16;
#undef M6_T
  return m == 0 ? W0 : m == 1 ? W1 : m == 2 ? W2 : m == 3 ? W3 : m == 4 ? W4 : W5;
}

DG_FN void m6_sqr(const uint32_t* it, int m, fp& re, fp& im) {
  const uint32_t w = m6_sqr_word(m);
  m6_term tm[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const uint32_t x = w >> (8 * t);
    tm[t].a = it + (x & 7u) * M6_COEF_WORDS;
    tm[t].b = it + ((x >> 3) & 7u) * M6_COEF_WORDS + ((x >> 6) & 1u) * 2 * ENG_SLOT_WORDS;
    tm[t].sh = (x >> 7) & 1u;
  }
  const uint32_t* sq = (w >> 27) & 1u ? it + ((w >> 24) & 7u) * M6_COEF_WORDS : nullptr;
  m6_fp2_sum<3, true>(tm, sq, re, im);
}

}  // namespace dgpu
