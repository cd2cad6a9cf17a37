// TEST-ONLY host build of the per-thread kernels' arithmetic in both forms of
// fp_reduce_lz (fp.cuh): the reduction straight from lazy limbs (LZ = true,
// shipped) against the carried form fp_reduce(fp_norm(x)) (LZ = false).
// tests/test_reduce_lazy_host.py builds it as a shared library; with
// -DRL_MAIN it is a stand-alone program (its own main, fixed inputs), which is
// the form to build with host sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../drand_amd/csrc/h2c.cuh"
#include "../../drand_amd/csrc/pairing.cuh"
#define DG_NO_KERNELS
#include "../../drand_amd/csrc/lines_thread.cuh"
#include "../../drand_amd/csrc/kb_thread.cuh"

using namespace dgpu;

namespace {
// canonical (non-Montgomery) residue of a CI value
fp canon(const fp& a) { return fp_from_mont(a); }
bool same(const fp& a, const fp& b) {
  const fp x = canon(a), y = canon(b);
  return !memcmp(&x, &y, sizeof(fp));
}
bool same2(const fp2& a, const fp2& b) { return same(a.c0, b.c0) && same(a.c1, b.c1); }
// CI: limbs < 2^28 and value < 2.01p (top limb < floor(2.01 floor(p / 2^364)) = 214,091,
// which bounds the value by 2.01p)
bool ci(const fp& a) {
  for (int i = 0; i < FP_LIMBS; ++i)
    if (a.l[i] > FP_MASK) return false;
  return a.l[FP_LIMBS - 1] < 214091u;
}
bool ci2(const fp2& a) { return ci(a.c0) && ci(a.c1); }

// fp_norm with 64-bit carries: fp_norm wherever fp_norm is defined (limbs
// < 2^31), and exact for any limbs < 2^32 with value < 2^392.
fp norm64(const fp& a) {
  fp r;
  uint64_t c = 0;
  for (int i = 0; i < FP_LIMBS - 1; ++i) {
    const uint64_t s = (uint64_t)a.l[i] + c;
    r.l[i] = (uint32_t)s & FP_MASK;
    c = s >> FP_BITS;
  }
  r.l[FP_LIMBS - 1] = (uint32_t)((uint64_t)a.l[FP_LIMBS - 1] + c);
  return r;
}

// f^((p^6 - 1)(p^2 + 1)): into the cyclotomic subgroup
fp12 easy_part(const fp12& f) {
  const fp12 t = fp12_mul(fp12_conj(f), fp12_inv(f));
  return fp12_mul(fp12_frob2(t), t);
}

// 63 compressed squarings of m's (f1, f2, f4, f5) in both forms, side by side
// with fp12_cyclo_sqr of the whole element: 0, or the first failing squaring
// (1-based; + 100 if CI failed, + 200 if the forms differ, + 300 if the
// new form differs from fp12_cyclo_sqr's components; that check only with
// `cyclo`, for m in the cyclotomic subgroup).
int kb_run(const fp12& m, bool cyclo = true) {
  // w-basis coefficients 1, 2, 4, 5 (tower.cuh: w -> c1.c0, w^2 -> c0.c1, w^4 -> c0.c2, w^5 -> c1.c2)
  fp2 a1 = m.c1.c0, a2 = m.c0.c1, a4 = m.c0.c2, a5 = m.c1.c2;
  fp2 b1 = a1, b2 = a2, b4 = a4, b5 = a5;
  fp12 g = m;
  for (int s = 1; s <= 63; ++s) {
    kb_sqr_thr<true>(a1, a2, a4, a5);
    kb_sqr_thr<false>(b1, b2, b4, b5);
    g = fp12_cyclo_sqr(g);
    if (!ci2(a1) || !ci2(a2) || !ci2(a4) || !ci2(a5)) return 100 + s;
    if (!same2(a1, b1) || !same2(a2, b2) || !same2(a4, b4) || !same2(a5, b5)) return 200 + s;
    if (cyclo && (!same2(a1, g.c1.c0) || !same2(a2, g.c0.c1) || !same2(a4, g.c0.c2) || !same2(a5, g.c1.c2))) return 300 + s;
  }
  return 0;
}

struct coeffs {
  std::vector<fp2> v;
  g2p T;
};
template <bool LZ>
coeffs lines_run(const g2a& Q, const fp& nx, const fp& y) {
  coeffs c;
  c.T = lt_pair_p<LZ>(lt_q_val{Q}, lt_pt_val{nx, y}, [&](int, int, const fp2& v) { c.v.push_back(v); });
  return c;
}
// one pair's 68 T-steps in both forms: 0, or 1 + the first differing
// coefficient's index (3 per step), 1000 a wrong count, 2000 the final T
int lines_pair(const g2a& Q, const fp& nx, const fp& y) {
  const coeffs a = lines_run<true>(Q, nx, y), b = lines_run<false>(Q, nx, y);
  if (a.v.size() != 3 * 68 || b.v.size() != a.v.size()) return 1000;
  for (size_t i = 0; i < a.v.size(); ++i)
    if (!same2(a.v[i], b.v[i]) || !ci2(a.v[i])) return 1 + (int)i;
  if (!same2(a.T.x, b.T.x) || !same2(a.T.y, b.T.y) || !same2(a.T.z, b.T.z)) return 2000;
  return 0;
}

bool pairs_of(const uint8_t* pk48, const uint8_t* prev, uint32_t prev_len, uint64_t round, const uint8_t* sig96, g1a& pk,
              g2a& h, g2a& s) {
  if (g1_decompress(&pk, pk48, GROUP_ORDER_WORDS) != DEC_OK) return false;
  if (g2_decompress(&s, sig96, true) != DEC_OK) return false;
  uint32_t m[8];
  drand_digest(m, prev, prev_len, round);
  h = g2_to_affine(hash_to_g2(m));
  return true;
}
}  // namespace

extern "C" {

// n limb vectors x (14 words each, any limbs < 2^32, value < 2^392):
// lz[i] = fp_reduce_lz(x_i), ref[i] = fp_reduce(norm(x_i)), both as they come
// out (14 words), and canon_lz / canon_ref their canonical non-Montgomery
// residues.  Returns the number of i whose residues differ or whose lz output
// is not CI.
int rl_reduce(const uint32_t* x, int n, uint32_t* lz, uint32_t* ref, uint32_t* canon_lz, uint32_t* canon_ref) {
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    fp a;
    memcpy(a.l, x + (size_t)i * FP_LIMBS, sizeof a.l);
    const fp r = fp_reduce_lz<true>(a), q = fp_reduce(norm64(a));
    const fp cr = canon(r), cq = canon(q);
    memcpy(lz + (size_t)i * FP_LIMBS, r.l, sizeof r.l);
    memcpy(ref + (size_t)i * FP_LIMBS, q.l, sizeof q.l);
    memcpy(canon_lz + (size_t)i * FP_LIMBS, cr.l, sizeof cr.l);
    memcpy(canon_ref + (size_t)i * FP_LIMBS, cq.l, sizeof cq.l);
    if (memcmp(&cr, &cq, sizeof cr) || !ci(r)) ++bad;
  }
  return bad;
}

// kb_sqr_thr in both forms from n seeded elements of the cyclotomic subgroup
// (the easy part of random Fp12 elements): the number of failing starts;
// *first = kb_run's code of the first failure.
int rl_kb_random(int n, uint64_t seed, int* first) {
  uint64_t s = seed | 1;
  auto rnd = [&]() {
    fp x;
    for (int i = 0; i < FP_LIMBS; ++i) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      x.l[i] = (uint32_t)s & FP_MASK;
    }
    x.l[FP_LIMBS - 1] &= 0x3FFFFFu;
    return fp_reduce(x);
  };
  int bad = 0;
  *first = 0;
  for (int t = 0; t < n; ++t) {
    fp12 f;
    fp* c = reinterpret_cast<fp*>(&f);
    for (int k = 0; k < 12; ++k) c[k] = rnd();
    const int rc = kb_run(easy_part(f));
    if (rc && !bad) *first = rc;
    bad += rc != 0;
  }
  return bad;
}

// The largest CI start: every limb 2^28 - 1 under the largest top limb the CI
// check admits (value just under 2.01p) in all eight coordinates, where the
// lazy sums' limbs come closest to 2^32.  kb_run's code (forms and CI only).
int rl_kb_edge() {
  fp mx;
  for (int i = 0; i < FP_LIMBS; ++i) mx.l[i] = FP_MASK;
  mx.l[FP_LIMBS - 1] = 214090u;
  fp12 f;
  fp* c = reinterpret_cast<fp*>(&f);
  for (int k = 0; k < 12; ++k) c[k] = mx;
  return kb_run(f, false);
}

// The five chain inputs of one verification's final exponentiation (pairs
// (pk, H(prev, round)) and (-g1, sig)): the number of failing chains (< 0: the
// inputs did not decode); *first as above.
int rl_kb_golden(const uint8_t* pk48, const uint8_t* prev, uint32_t prev_len, uint64_t round, const uint8_t* sig96,
                 int* first) {
  g1a pk;
  g2a h, s;
  if (!pairs_of(pk48, prev, prev_len, round, sig96, pk, h, s)) return -1;
  const fp12 f = miller_loop_2(h, fp_neg(pk.x), pk.y, s, fp_neg(C_G1_X), C_G1_NEG_Y);
  const fp12 t = easy_part(f);
  const fp12 t0 = fp12_mul(fp12_exp_x(t), fp12_conj(t));
  const fp12 t1 = fp12_mul(fp12_exp_x(t0), fp12_conj(t0));
  const fp12 t2 = fp12_mul(fp12_exp_x(t1), fp12_frob1(t1));
  const fp12 in[5] = {t, t0, t1, t2, fp12_exp_x(t2)};
  int bad = 0;
  *first = 0;
  for (const fp12& m : in) {
    const int rc = kb_run(m);
    if (rc && !bad) *first = rc;
    bad += rc != 0;
  }
  return bad;
}

// The 68 T-steps of both pairs of one verification in both forms: 0, or
// 10000 * (pair + 1) + lines_pair's code (< 0: the inputs did not decode).
int rl_lines_golden(const uint8_t* pk48, const uint8_t* prev, uint32_t prev_len, uint64_t round, const uint8_t* sig96) {
  g1a pk;
  g2a h, s;
  if (!pairs_of(pk48, prev, prev_len, round, sig96, pk, h, s)) return -1;
  int rc = lines_pair(h, fp_neg(pk.x), pk.y);
  if (rc) return 10000 + rc;
  rc = lines_pair(s, fp_neg(C_G1_X), C_G1_NEG_Y);
  return rc ? 20000 + rc : 0;
}
}

#ifdef RL_MAIN
// Stand-alone run on fixed inputs: seeded limb vectors through rl_reduce, the
// seeded chains, and the T-steps of a pair made from hashed points.
int main() {
  const int n = 20000;
  std::vector<uint32_t> x((size_t)n * FP_LIMBS), o((size_t)4 * n * FP_LIMBS);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < n; ++i)
    for (int l = 0; l < FP_LIMBS; ++l) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      x[(size_t)i * FP_LIMBS + l] = l == FP_LIMBS - 1 ? (uint32_t)s & 0x0FFFFFEFu : (uint32_t)s;  // value < 2^392
    }
  const size_t k = (size_t)n * FP_LIMBS;
  int bad = rl_reduce(x.data(), n, o.data(), o.data() + k, o.data() + 2 * k, o.data() + 3 * k);
  printf("rl_reduce: %d bad of %d\n", bad, n);
  int first = 0;
  const int kb = rl_kb_random(8, 7, &first);
  printf("rl_kb_random: %d bad (first %d), edge %d\n", kb, first, rl_kb_edge());
  uint32_t m0[8] = {1, 2, 3, 4, 5, 6, 7, 8}, m1[8] = {8, 7, 6, 5, 4, 3, 2, 1};
  const g2a q0 = g2_to_affine(hash_to_g2(m0)), q1 = g2_to_affine(hash_to_g2(m1));
  const int l0 = lines_pair(q0, fp_neg(C_G1_X), C_G1_NEG_Y), l1 = lines_pair(q1, fp_neg(C_G1_X), C_G1_NEG_Y);
  printf("lines_pair: %d %d\n", l0, l1);
  return bad || kb || rl_kb_edge() || l0 || l1;
}
#endif
