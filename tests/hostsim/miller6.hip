// TEST-ONLY host build of the six-lane Miller arithmetic (miller6.cuh): the
// lanes of one item emulated over an array, against tower.cuh's Fp12
// arithmetic.  tests/test_miller6_host.py builds it as a shared library; with
// -DM6_MAIN it is a stand-alone program (its own main, fixed inputs), which is
// the form to build with host sanitizers.
//
// It is built on top of hostsim.hip (included as it is): HostGroup and
// host_exec run the 12-lane ENG_PROG_MILLER on the host, the reference for the
// whole loop's f and N1.
#include <cstdio>
#include "hostsim.hip"
#include "../../drand_amd/csrc/miller6.cuh"

using namespace dgpu;

namespace {
fp canon(const fp& a) { return fp_from_mont(a); }
bool same(const fp& a, const fp& b) {
  const fp x = canon(a), y = canon(b);
  return !memcmp(&x, &y, sizeof(fp));
}
// w-basis coefficient k of an fp12 (tower.cuh: 1 -> c0.c0, w -> c1.c0, w^2 -> c0.c1, ...)
const fp2& coef(const fp12& f, int k) {
  const fp6& h = (k & 1) ? f.c1 : f.c0;
  return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
// what the kernel keeps in LDS: limbs < 2^28, value < 2.3p (top limb < 2.3 floor(p / 2^364))
bool stored_ok(const fp& a) {
  for (int i = 0; i < FP_LIMBS; ++i)
    if (a.l[i] > FP_MASK) return false;
  return a.l[FP_LIMBS - 1] < 244982u;
}

struct item {
  uint32_t w[M6_ITEM_WORDS];
};
void put_f(item& it, const fp12& f) {
  for (int m = 0; m < 6; ++m) m6_store(it.w, m, coef(f, m).c0, coef(f, m).c1);
}
void put_line(item& it, int line, const fp2& l0, const fp2& l2, const fp2& l3) {
  const fp2 l[3] = {l0, l2, l3};
  for (int t = 0; t < 3; ++t) {
    eng_st(it.w + (line + 2 * t) * ENG_SLOT_WORDS, l[t].c0);
    eng_st(it.w + (line + 2 * t + 1) * ENG_SLOT_WORDS, l[t].c1);
  }
}
// one op on all six lanes: every lane reads before any lane writes
template <class F>
bool run_op(item& it, F&& op) {
  fp re[6], im[6];
  for (int m = 0; m < 6; ++m) op(it.w, m, re[m], im[m]);
  bool ok = true;
  for (int m = 0; m < 6; ++m) {
    ok = ok && stored_ok(re[m]) && stored_ok(im[m]);
    m6_store(it.w, m, re[m], im[m]);
  }
  return ok;
}
bool matches(const item& it, const fp12& f) {
  for (int m = 0; m < 6; ++m) {
    const uint32_t* p = it.w + m * M6_COEF_WORDS;
    const fp2 x = fp2_mul_xi(coef(f, m));
    if (!same(eng_ld(p), coef(f, m).c0) || !same(eng_ld(p + ENG_SLOT_WORDS), coef(f, m).c1) ||
        !same(eng_ld(p + 2 * ENG_SLOT_WORDS), x.c0) || !same(eng_ld(p + 3 * ENG_SLOT_WORDS), x.c1))
      return false;
  }
  return true;
}

// `steps` doubling steps f <- f^2 l1 l2 from f and the two lines, both ways:
// 0, or 10 * step + (1 squaring, 2 line 1, 3 line 2; + 4 if a stored value is out of range)
int run_steps(const fp12& f0, const fp2* l1, const fp2* l2, int steps) {
  item it;
  memset(&it, 0, sizeof it);
  put_f(it, f0);
  put_line(it, M6_L1, l1[0], l1[1], l1[2]);
  put_line(it, M6_L2, l2[0], l2[1], l2[2]);
  fp12 f = f0;
  for (int s = 1; s <= steps; ++s) {
    bool ok = run_op(it, [](const uint32_t* w, int m, fp& re, fp& im) { m6_sqr(w, m, re, im); });
    f = fp12_sqr(f);
    if (!ok || !matches(it, f)) return 10 * s + 1 + (ok ? 0 : 4);
    ok = run_op(it, [](const uint32_t* w, int m, fp& re, fp& im) { m6_line_mul(w, m, M6_L1, re, im); });
    f = fp12_mul_line(f, l1[0], l1[1], l1[2]);
    if (!ok || !matches(it, f)) return 10 * s + 2 + (ok ? 0 : 4);
    ok = run_op(it, [](const uint32_t* w, int m, fp& re, fp& im) { m6_line_mul(w, m, M6_L2, re, im); });
    f = fp12_mul_line(f, l2[0], l2[1], l2[2]);
    if (!ok || !matches(it, f)) return 10 * s + 3 + (ok ? 0 : 4);
  }
  return 0;
}

// k_eng_miller6 over the line buffer of `cnt` items, its waves' 64 lanes in
// lockstep (every lane of an op reads before any lane writes), with the
// kernel's own address and schedule functions: f -> fbuf plane 0.  Returns the
// largest word offset read in `lines` (*max_f: written in fbuf).
size_t run_kernel(size_t cnt, const uint32_t* lines, uint32_t* fbuf, size_t* max_f) {
  size_t max_l = 0;
  *max_f = 0;
  const size_t waves = (cnt + M6_ITEMS_PER_WAVE - 1) / M6_ITEMS_PER_WAVE;
  std::vector<uint32_t> lds(M6_ITEMS_PER_WAVE * M6_ITEM_WORDS);
  for (size_t w = 0; w < waves; ++w) {
    m6_lane L[64];
    fp re[64], im[64];
    for (int t = 0; t < 64; ++t) L[t] = m6_lane_id(cnt, w, t);
    auto item = [&](int t) { return lds.data() + L[t].gi * M6_ITEM_WORDS; };
    auto store_all = [&]() {
      for (int t = 0; t < 64; ++t) m6_store(item(t), L[t].m, re[t], im[t]);
    };
    for (int t = 0; t < 64; ++t) re[t] = L[t].m == 0 ? fp_one() : fp_zero(), im[t] = fp_zero();
    store_all();
    m6_sched sc;
    for (int step = 0; step < ENG_LINE_STEPS; ++step) {
      if (m6_sched_sqr(sc)) {
        for (int t = 0; t < 64; ++t) m6_sqr(item(t), L[t].m, re[t], im[t]);
        store_all();
      }
      for (int t = 0; t < 64; ++t) {
        const size_t off = m6_line_off(L[t], step);
        fp a, b;
        for (int l = 0; l < FP_LIMBS; ++l) a.l[l] = lines[off + l * ENG_WAVE_WORDS], b.l[l] = lines[off + l * ENG_WAVE_WORDS + 1];
        if (off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 1 > max_l) max_l = off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 1;
        eng_st(item(t) + (M6_L1 + 2 * L[t].m) * ENG_SLOT_WORDS, a);
        eng_st(item(t) + (M6_L1 + 2 * L[t].m + 1) * ENG_SLOT_WORDS, b);
      }
      for (int line = M6_L1; line <= M6_L2; line += M6_L2 - M6_L1) {
        for (int t = 0; t < 64; ++t) m6_line_mul(item(t), L[t].m, line, re[t], im[t]);
        store_all();
      }
      m6_sched_next(sc);
    }
    for (int t = 0; t < 64; ++t) {
      if (!L[t].valid) continue;
      const fp a = eng_reduce(eng_ld(item(t) + L[t].m * M6_COEF_WORDS));
      const fp b = eng_reduce(eng_ld(item(t) + L[t].m * M6_COEF_WORDS + ENG_SLOT_WORDS));
      const size_t off = m6_f_off(L[t]);
      for (int l = 0; l < FP_LIMBS; ++l) fbuf[off + l * ENG_WAVE_WORDS] = a.l[l], fbuf[off + l * ENG_WAVE_WORDS + 1] = b.l[l];
      if (off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 1 > *max_f) *max_f = off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 1;
    }
  }
  return max_l;
}
}  // namespace

extern "C" {

// The line buffer of `cnt` copies of one verification's two pairs ((pk, H) and
// (-g1, sigma), k_lines_thr's coefficients in its layout) through the emulated
// kernel: every item's f must be slot values (limbs < 2^28, < 2.01p) with the
// canonical residues of the tower's product of the same lines (fp12_sqr,
// fp12_mul_line), and the canonical residues of the 12-lane program's f
// (ENG_PROG_MILLER through hostsim.hip's host_exec, whose schedule is the
// program's own); N1, formed from the emulated kernel's f as
// k_eng_miller_tail forms it, must be the whole program's N1.  0, or 1 + the
// first failing item against the tower, 1000 + against the program's f, 2000 +
// its N1, 3000 + if the tail changed f (< 0: the inputs did not decode, or an
// address left its buffer).
int m6_golden(const uint8_t* pk48, const uint8_t* prev, uint32_t prev_len, uint64_t round, const uint8_t* sig96, int cnt) {
  g1a pk;
  g2a h, sg;
  if (g1_decompress(&pk, pk48, GROUP_ORDER_WORDS) != DEC_OK || g2_decompress(&sg, sig96, true) != DEC_OK) return -1;
  uint32_t dm[8];
  drand_digest(dm, prev, prev_len, round);
  h = g2_to_affine(hash_to_g2(dm));
  std::vector<fp2> lc(2 * ENG_LINE_STEPS * 3);  // [pair][step][k]
  lt_pair_p(lt_q_val{h}, lt_pt_val{fp_neg(pk.x), pk.y}, [&](int step, int k, const fp2& v) { lc[step * 3 + k] = v; });
  lt_pair_p(lt_q_val{sg}, lt_pt_val{fp_neg(C_G1_X), C_G1_NEG_Y},
            [&](int step, int k, const fp2& v) { lc[(ENG_LINE_STEPS + step) * 3 + k] = v; });
  fp12 f = fp12_one();
  m6_sched sc;
  for (int step = 0; step < ENG_LINE_STEPS; ++step) {
    if (m6_sched_sqr(sc)) f = fp12_sqr(f);
    for (int p = 0; p < 2; ++p) {
      const fp2* l = &lc[(p * ENG_LINE_STEPS + step) * 3];
      f = fp12_mul_line(f, l[0], l[1], l[2]);
    }
    m6_sched_next(sc);
  }
  const size_t nblk = eng_blocks((size_t)cnt);
  const size_t lw = eng_blk_words(nblk, ENG_LINE_STEPS), fw = eng_blk_words(nblk, ENG_F_PLANES);
  std::vector<uint32_t> lines(lw, 0u), fbuf(fw, 0xEEEEEEEEu);
  for (int i = 0; i < cnt; ++i)
    for (int p = 0; p < 2; ++p)
      for (int step = 0; step < ENG_LINE_STEPS; ++step)
        for (int k = 0; k < 3; ++k) {
          const fp2& v = lc[(p * ENG_LINE_STEPS + step) * 3 + k];
          const size_t off = eng_blk_off(i / ENG_ROUNDS_PER_BLOCK, ENG_LINE_STEPS, step, i % ENG_ROUNDS_PER_BLOCK, 6 * p + 2 * k);
          for (int l = 0; l < FP_LIMBS; ++l) lines[off + l * ENG_WAVE_WORDS] = v.c0.l[l], lines[off + l * ENG_WAVE_WORDS + 1] = v.c1.l[l];
        }
  size_t max_f = 0;
  const size_t max_l = run_kernel((size_t)cnt, lines.data(), fbuf.data(), &max_f);
  if (max_l > lw || max_f > fw) return -2;
  for (int i = 0; i < cnt; ++i)
    for (int m = 0; m < 6; ++m) {
      const size_t off = eng_blk_off(i / ENG_ROUNDS_PER_BLOCK, ENG_F_PLANES, 0, i % ENG_ROUNDS_PER_BLOCK, 2 * m);
      fp a, b;
      for (int l = 0; l < FP_LIMBS; ++l) a.l[l] = fbuf[off + l * ENG_WAVE_WORDS], b.l[l] = fbuf[off + l * ENG_WAVE_WORDS + 1];
      const bool ci = stored_ok(a) && stored_ok(b) && a.l[FP_LIMBS - 1] < 214091u && b.l[FP_LIMBS - 1] < 214091u;
      if (!ci || !same(a, coef(f, m).c0) || !same(b, coef(f, m).c1)) return 1 + i;
    }
  // rounds past cnt in the last block stay unwritten
  for (size_t i = (size_t)cnt; i < nblk * ENG_ROUNDS_PER_BLOCK; ++i)
    if (fbuf[eng_blk_off(i / ENG_ROUNDS_PER_BLOCK, ENG_F_PLANES, 0, (int)(i % ENG_ROUNDS_PER_BLOCK), 0)] != 0xEEEEEEEEu) return -3;
  // The 12-lane program over the same lines (hostsim.hip host_exec: its own
  // schedule, from ENG_PROG_MILLER): f and N1 of k_eng_miller.
  static HostGroup G;
  G = HostGroup();
  host_consts(G, pk);
  for (int p = 0; p < 2; ++p)
    for (int step = 0; step < ENG_LINE_STEPS; ++step)
      for (int k = 0; k < 3; ++k) {
        const fp2& v = lc[(p * ENG_LINE_STEPS + step) * 3 + k];
        G.lines[step * 12 + 6 * p + 2 * k] = v.c0, G.lines[step * 12 + 6 * p + 2 * k + 1] = v.c1;
      }
  for (int k = 0; k < 12; ++k) G.set(ENG_M_F + k, k == 0 ? fp_one() : fp_zero());
  G.step = 0;
  host_exec(G, ENG_PROG_MILLER, ENG_PROG_MILLER_LEN);
  for (int i = 0; i < cnt; ++i) {
    // k_eng_miller_tail: a fresh group (garbage in every slot), the constants,
    // f from fbuf's plane 0, the program's last ENG_MILLER_TAIL_OPS ops
    static HostGroup T;
    T = HostGroup();
    host_scramble(T, 0x9E3779B97F4A7C15ull + (uint64_t)i);
    host_consts(T, pk);
    for (int k = 0; k < 12; ++k) {
      const size_t off = eng_blk_off(i / ENG_ROUNDS_PER_BLOCK, ENG_F_PLANES, 0, i % ENG_ROUNDS_PER_BLOCK, k);
      fp a;
      for (int l = 0; l < FP_LIMBS; ++l) a.l[l] = fbuf[off + l * ENG_WAVE_WORDS];
      if (!same(a, G.get(ENG_M_F + k))) return 1000 + i;  // f differs from the 12-lane program's
      T.set(ENG_M_F + k, a);
    }
    T.n1 = fp_zero();
    host_exec(T, ENG_PROG_MILLER + ENG_PROG_MILLER_LEN - ENG_MILLER_TAIL_OPS, ENG_MILLER_TAIL_OPS);
    if (!same(T.n1, G.n1)) return 2000 + i;  // N1 differs
    for (int k = 0; k < 12; ++k)
      if (!same(T.get(ENG_M_F + k), G.get(ENG_M_F + k))) return 3000 + i;  // the tail changed f
  }
  return 0;
}

// The addresses of k_eng_miller6 for `cnt` items, without the arithmetic: one
// past the largest word its lanes read in the line buffer and write in the f
// buffer (out[0], out[1]) and the buffers' sizes eng_blk_words(eng_blocks(cnt), .)
// (out[2], out[3]); out[4] = 1 if some lane's two words are not 8-byte aligned.
void m6_extents(uint64_t cnt, uint64_t* out) {
  size_t max_l = 0, max_f = 0;
  bool odd = false;
  const size_t waves = (cnt + M6_ITEMS_PER_WAVE - 1) / M6_ITEMS_PER_WAVE;
  for (size_t w = 0; w < waves; ++w)
    for (int t = 0; t < 64; ++t) {
      const m6_lane L = m6_lane_id(cnt, w, t);
      for (int step = 0; step < ENG_LINE_STEPS; ++step) {
        const size_t off = m6_line_off(L, step);
        odd = odd || (off & 1);
        if (off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 2 > max_l) max_l = off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 2;
      }
      if (L.valid) {
        const size_t off = m6_f_off(L);
        odd = odd || (off & 1);
        if (off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 2 > max_f) max_f = off + (FP_LIMBS - 1) * ENG_WAVE_WORDS + 2;
      }
    }
  out[0] = max_l, out[1] = max_f;
  out[2] = eng_blk_words(eng_blocks(cnt), ENG_LINE_STEPS), out[3] = eng_blk_words(eng_blocks(cnt), ENG_F_PLANES);
  out[4] = odd;
}

// n seeded starts (f and two lines random, values CI), `steps` doubling steps
// each: the number of failing starts; *first = run_steps' code of the first.
int m6_random(int n, uint64_t seed, int steps, int* first) {
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
    fp2 l1[3], l2[3];
    for (int k = 0; k < 3; ++k) l1[k] = fp2{rnd(), rnd()}, l2[k] = fp2{rnd(), rnd()};
    const int rc = run_steps(f, l1, l2, steps);
    if (rc && !bad) *first = rc;
    bad += rc != 0;
  }
  return bad;
}

// Operands at the limb maxima of a stored value (every limb 2^28 - 1 under the
// top limb of 2.3p), in f and in both lines, three doubling steps each:
//   0  re = im = maximum (re + im at its bound)
//   1  re = maximum, im = 0 (re - im + 8p at its bound, 10.3p: the wrapped terms' operand)
//   2  re = 0, im = maximum (its mirror: re - im + 8p smallest, the products' im parts largest)
// (the first step runs on these operands; the later ones on what it leaves).
// 0, or 100 * (1 + case) + run_steps' code.
int m6_edge() {
  fp mx;
  for (int i = 0; i < FP_LIMBS; ++i) mx.l[i] = FP_MASK;
  mx.l[FP_LIMBS - 1] = 244981u;
  const fp z = fp_zero();
  const fp2 pat[3] = {fp2{mx, mx}, fp2{mx, z}, fp2{z, mx}};
  for (int cs = 0; cs < 3; ++cs) {
    fp12 f;
    fp2* c = reinterpret_cast<fp2*>(&f);
    for (int k = 0; k < 6; ++k) c[k] = pat[cs];
    const fp2 l[3] = {pat[cs], pat[cs], pat[cs]};
    const int rc = run_steps(f, l, l, 3);
    if (rc) return 100 * (1 + cs) + rc;
  }
  return 0;
}
}

#ifdef M6_MAIN
int main() {
  int first = 0;
  const int bad = m6_random(64, 7, 3, &first);
  const int edge = m6_edge();
  printf("m6_random: %d bad (first %d), edge %d\n", bad, first, edge);
  int ext = 0;
  for (uint64_t cnt : {1, 4, 5, 6, 9, 10, 11, 63, 64, 65}) {
    uint64_t o[5];
    m6_extents(cnt, o);
    ext += o[0] > o[2] || o[1] > o[3] || o[4];
  }
  printf("m6_extents: %d bad\n", ext);
  return bad || edge || ext;
}
#endif
