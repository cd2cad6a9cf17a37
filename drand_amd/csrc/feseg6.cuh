// The Karabina FE's segments 1..5 (tools/gen_engine.py prog_fe_kb) with one
// Fp2 coefficient per lane: miller6.cuh's lane model
// for the Fp12 products E_MUL / E_MULCJ.  Six lanes cooperate on one item,
// lane m owns coefficient m of R = sum R_m w^m and of the operand A, ten items
// per wave (m6_lane_id's addressing).  An Fp2 product takes 3 Fp product terms
// by Karatsuba (m6_fp2_sum) where the 12-lane ops take 4: 6 lanes x (6 x 3
// terms + 2 reductions) = 120 units per Fp12 product against 144 + 12.
//
// Item state in LDS, M6_SLOTS = 36 slots of 14 words (2,016 bytes):
//   slot 4m + 0..3      R_m as (re, im, re - im + 8p, re + im), written by the
//                       owning lane with m6_store (the last two are xi R_m)
//   slot FS6_A + 2m, +1 A_m as (re, im)
// Every stored value has normalized limbs (< 2^28 below the top limb).
//
// Product: lane m forms
//   c_m = sum_{i + j = m} R_i A_j + sum_{i + j = m + 6} (xi R_i) A_j
// as one six-term m6_fp2_sum (miller6.cuh: U, S, W and the two reductions).
//
// Column bounds (limbs of stored values < 2^28, top limbs < 2^21; a column has
// at most 13 full-size products):
//   |U - S| < 6 * 13 * 2^56 < 2^62.3               (< 2^63 - 2^60, signed)
//   W - (U + S) < 12 * 13 * 2^56 < 2^63.3          (< 2^64 - 2^60)
// W's own columns (operand sums, limbs < 2^29) may wrap 2^64; the difference
// is exact modulo 2^64 and below the bound above (miller6.cuh).
// Values: R_i and A_j are below 2.3p, so a term's operands are below
// (10.3p, 4.6p; sum 12.6p) and (2.3p, 2.3p; sum 4.6p), and U, S and W are
// below 6 * 12.6p * 4.6p < 348 p^2 (inside the 568 p^2 < 0.26 p R the lane
// model allows): both outputs are below 2.3p with normalized limbs.
//
// Glue, per coefficient (the semantics of gen_engine.build_ops' E_CONJ, conj_a
// of E_MULCJ, E_FROB1, E_FROB2, E_CYCA):
//   conj       negate the odd-m coefficients (fs6_neg: 8p - x, carried, reduced)
//   frob1      A_m <- conj(A_m) * gamma_1,m,  frob2  A_m <- A_m * gamma_2,m
//              (block constants ENG_C_G1 / ENG_C_G2; gamma_.,0 = 1)
//   A <- A^2   m6_sqr (the general squaring: same residue as the cyclotomic
//              one) on A parked in R's slots while the lane holds R_m in
//              registers
// Values that go to a state plane are reduced first (< 2.01p, what the planes'
// readers expect).
#pragma once
#include "miller6.cuh"

namespace dgpu {

constexpr int FS6_A = 24;  // first slot of the operand A
static_assert(FS6_A + 2 * M6_LANES == M6_SLOTS, "R takes 6 x 4 slots, A 6 x 2");

// ---------------------------------------------------------------- the segments' schedule
// Segment e = 1..5 as products R <- R * A: step s loads A from `plane` (or
// squares the A it has: FS6_X_SQR), transforms it, multiplies, then conjugates
// and stores R as the flags say.  R starts as plane X0.
enum { FS6_X_NONE = 0, FS6_X_CONJ = 1, FS6_X_FROB1 = 2, FS6_X_FROB2 = 3, FS6_X_SQR = 4 };
struct fs6_step {
  int plane, xf;
  bool conj_r, st_m, st_t2;
};
constexpr int FS6_LAST_SEG = (int)(sizeof(ENG_PROG_FEK_OFF) / sizeof(ENG_PROG_FEK_OFF[0])) - 2;  // ends with R = FE(f)
static_assert(FS6_LAST_SEG == 5, "segment 0, then one per exponentiation by |x|");
DG_FN int fs6_nsteps(int seg) { return seg == 4 ? 5 : seg == FS6_LAST_SEG ? 9 : 6; }
DG_FN fs6_step fs6_plan(int seg, int s) {
  fs6_step p{0, FS6_X_NONE, false, false, false};
  if (s < ENG_KB_NSNAP - 1) {  // m^|x|: the product of the six decompressed values, conjugated to m^x
    p.plane = ENG_KB_PL_X0 + 1 + s;
    p.conj_r = s == ENG_KB_NSNAP - 2;
    p.st_m = p.conj_r && seg == 4;  // t2^x
    return p;
  }
  const int q = s - (ENG_KB_NSNAP - 1);
  if (seg == 1 || seg == 2) {  // t0 = t^x conj(t), t1 = t0^x conj(t0)
    p.plane = ENG_KB_PL_M, p.xf = FS6_X_CONJ, p.st_m = true;
  } else if (seg == 3) {  // t2 = t1^x t1^p
    p.plane = ENG_KB_PL_M, p.xf = FS6_X_FROB1, p.st_m = p.st_t2 = true;
  } else {  // t3 = t2^(x^2) t2^(p^2) conj(t2), times t^3 = t t^2
    p.plane = q < 2 ? ENG_KB_PL_T2 : ENG_KB_PL_T;
    p.xf = q == 0 ? FS6_X_FROB2 : q == 1 ? FS6_X_CONJ : q == 2 ? FS6_X_NONE : FS6_X_SQR;
  }
  return p;
}

// ---------------------------------------------------------------- addressing
// Lane m moves components 2m and 2m + 1 of its item's state plane as one
// dwordx2 per limb (kb_off(i, plane, 2m), as kb_ld2 / kb_st2 do); limb l is
// l * ENG_WAVE_WORDS further.  With an odd number of blocks the last wave's
// second half reads the last block again and writes nothing (m6_lane_id).
DG_FN size_t fs6_plane_off(const m6_lane& L, int plane) { return eng_blk_off(L.blk, ENG_KB_PLANES, plane, L.g, 2 * L.m); }
// the item's chunk-local index (valid lanes)
DG_FN size_t fs6_item(const m6_lane& L) { return L.blk * ENG_ROUNDS_PER_BLOCK + L.g; }

DG_FN fp2 fs6_ld_plane(const uint32_t* p) {
  fp2 v;
#pragma unroll
  for (int l = 0; l < FP_LIMBS; ++l) {
    const uint2 w = *reinterpret_cast<const uint2*>(p + l * ENG_WAVE_WORDS);
    v.c0.l[l] = w.x, v.c1.l[l] = w.y;
  }
  return v;
}
// v below 2.3p -> the plane's values, below 2.01p
DG_FN void fs6_st_plane(uint32_t* p, const fp& re, const fp& im) {
  const fp a = eng_reduce(re), b = eng_reduce(im);
#pragma unroll
  for (int l = 0; l < FP_LIMBS; ++l) *reinterpret_cast<uint2*>(p + l * ENG_WAVE_WORDS) = make_uint2(a.l[l], b.l[l]);
}

DG_FN fp2 fs6_get_a(const uint32_t* it, int m) {
  const uint32_t* p = it + (FS6_A + 2 * m) * ENG_SLOT_WORDS;
  return fp2{eng_ld(p), eng_ld(p + ENG_SLOT_WORDS)};
}
DG_FN void fs6_put_a(uint32_t* it, int m, const fp2& a) {
  uint32_t* p = it + (FS6_A + 2 * m) * ENG_SLOT_WORDS;
  eng_st(p, a.c0);
  eng_st(p + ENG_SLOT_WORDS, a.c1);
}

// ---------------------------------------------------------------- glue
// -x for a normalized x below 7.99p: below 2.01p, normalized limbs
DG_FN fp fs6_neg(const fp& x) { return eng_reduce(eng_cyc_sum(fp_zero(), x, true)); }

DG_FN fp fs6_const(const uint32_t* consts, int slot) {
  fp a;
#pragma unroll
  for (int l = 0; l < FP_LIMBS; ++l) a.l[l] = consts[(slot - ENG_C_ONE) * ENG_SLOT_WORDS + l];
  return a;
}

// x g (CONJ: conj(x) g) for x below 2.3p and a block constant g below 1.01p,
// with -y as 8p - y limb-wise (limbs < 2^29.6): two product terms per part,
// columns < 2 * 14 * 2^57.6 < 2^62.5, sums below 11 p^2, outputs below 1.01p.
template <bool CONJ>
DG_FN fp2 fs6_mul_const(const fp2& x, const fp& g0, const fp& g1) {
  const fp nx1 = fp_sub_lz(fp_zero(), x.c1);
  uint64_t col[2 * FP_LIMBS];
  col[2 * FP_LIMBS - 1] = 0;
  fp2 r;
  m6_mac<true>(col, g0, x.c0);
  m6_mac<false>(col, g1, CONJ ? x.c1 : nx1);  // re = x0 g0 - (+-x1) g1
  r.c0 = fp_redc_cols(col);
  m6_mac<true>(col, g1, x.c0);
  m6_mac<false>(col, g0, CONJ ? nx1 : x.c1);  // im = x0 g1 + (+-x1) g0
  r.c1 = fp_redc_cols(col);
  return r;
}

// Lane m's A coefficient as step transform xf leaves it (xf != FS6_X_SQR).
DG_FN fp2 fs6_xform(const fp2& a, int xf, int m, const uint32_t* consts) {
  if (xf == FS6_X_CONJ) return (m & 1) ? fp2{fs6_neg(a.c0), fs6_neg(a.c1)} : a;
  if (xf == FS6_X_FROB1) {
    const fp g0 = fs6_const(consts, m ? ENG_C_G1 + 2 * (m - 1) : ENG_C_ONE);
    const fp g1 = m ? fs6_const(consts, ENG_C_G1 + 2 * (m - 1) + 1) : fp_zero();
    return fs6_mul_const<true>(a, g0, g1);
  }
  if (xf == FS6_X_FROB2) return fs6_mul_const<false>(a, fs6_const(consts, m ? ENG_C_G2 + (m - 1) : ENG_C_ONE), fp_zero());
  return a;
}

// ---------------------------------------------------------------- the product
// Lane m's coefficient of R * A: term i is R_i A_((m - i) mod 6), with xi R_i
// where i + j wraps past w^6.
DG_FN void fs6_mul(const uint32_t* it, int m, fp& re, fp& im) {
  m6_term tm[M6_LANES];
#pragma unroll
  for (int i = 0; i < M6_LANES; ++i) {
    const bool wrap = i > m;
    tm[i].a = it + i * M6_COEF_WORDS + (wrap ? 2 * ENG_SLOT_WORDS : 0);
    tm[i].b = it + (FS6_A + 2 * (m - i + (wrap ? M6_LANES : 0))) * ENG_SLOT_WORDS;
    tm[i].sh = 0;
  }
  m6_fp2_sum<M6_LANES, false>(tm, nullptr, re, im);
}

// x == K mod p for a normalized x below 2.3p and a constant K below p
DG_FN bool fs6_eq(const fp& x, const fp& K) { return fp_is_zero(eng_reduce(fp_norm(fp_sub_lz(x, K)))); }
// lane m's part of R == 1
DG_FN bool fs6_is_one(const fp& re, const fp& im, int m) { return fs6_eq(re, m == 0 ? fp_one() : fp_zero()) && fs6_eq(im, fp_zero()); }

}  // namespace dgpu
