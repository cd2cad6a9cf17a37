// TEST-ONLY host build of the six-lane FE segments (feseg6.cuh): the lanes of
// a wave emulated over arrays, against tower.cuh's Fp12 arithmetic and against
// hostsim.hip's emulation of the same ENG_PROG_FEK segment on the 12-lane
// engine.  tests/test_feseg6_host.py builds it as a shared library; with
// -DFS6_MAIN it is a stand-alone program (its own main, fixed inputs), which
// is the form to build with host sanitizers.
#include <cstdio>
#include "hostsim.hip"
#include "../../drand_amd/csrc/feseg6.cuh"

using namespace dgpu;

namespace {
constexpr uint32_t TOP_23P = 244982u;   // top limb of a value below 2.3p: what the kernel keeps in LDS
constexpr uint32_t TOP_201P = 214091u;  // ... below 2.01p: what it writes to a state plane
constexpr size_t LIMB_SPAN = (size_t)(FP_LIMBS - 1) * ENG_WAVE_WORDS;

bool same(const fp& a, const fp& b) {
  const fp x = fp_from_mont(fp_reduce(a)), y = fp_from_mont(fp_reduce(b));
  return !memcmp(&x, &y, sizeof(fp));
}
bool bounded(const fp& a, uint32_t top) {
  for (int i = 0; i < FP_LIMBS - 1; ++i)
    if (a.l[i] > FP_MASK) return false;
  return a.l[FP_LIMBS - 1] < top;
}
// w-basis coefficient k of an fp12 (tower.cuh: 1 -> c0.c0, w -> c1.c0, w^2 -> c0.c1, ...)
fp2& coef(fp12& f, int k) {
  fp6& h = (k & 1) ? f.c1 : f.c0;
  return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
fp12 reduced(fp12 f) {
  for (int k = 0; k < 6; ++k) coef(f, k) = fp2{fp_reduce(coef(f, k).c0), fp_reduce(coef(f, k).c1)};
  return f;
}

struct rng {
  uint64_t s;
  fp next() {
    fp x;
    for (int i = 0; i < FP_LIMBS; ++i) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      x.l[i] = (uint32_t)s & FP_MASK;
    }
    x.l[FP_LIMBS - 1] &= 0x3FFFFFu;
    return fp_reduce(x);
  }
  fp12 next12() {
    fp12 f;
    for (int k = 0; k < 6; ++k) coef(f, k) = fp2{next(), next()};
    return f;
  }
};

const uint32_t* block_consts() {
  static HostGroup G;
  host_consts(G, g1a{fp_zero(), fp_zero()});  // the Frobenius constants do not depend on the key
  return G.c;
}

struct item {
  uint32_t w[M6_ITEM_WORDS];
};
// R and A of one item as the kernel holds them; false if a value leaves its bound
bool put_r(item& it, fp12 r) {
  bool ok = true;
  for (int m = 0; m < 6; ++m) {
    ok = ok && bounded(coef(r, m).c0, TOP_23P) && bounded(coef(r, m).c1, TOP_23P);
    m6_store(it.w, m, coef(r, m).c0, coef(r, m).c1);
  }
  return ok;
}
bool put_a(item& it, fp12 a) {
  bool ok = true;
  for (int m = 0; m < 6; ++m) {
    ok = ok && bounded(coef(a, m).c0, TOP_23P) && bounded(coef(a, m).c1, TOP_23P);
    fs6_put_a(it.w, m, coef(a, m));
  }
  return ok;
}
bool equals(fp12 got, fp12 want) {
  for (int m = 0; m < 6; ++m)
    if (!same(coef(got, m).c0, coef(want, m).c0) || !same(coef(got, m).c1, coef(want, m).c1)) return false;
  return true;
}
// R * A on the six lanes (every lane reads before any lane writes)
fp12 lanes_mul(const item& it) {
  fp12 c;
  for (int m = 0; m < 6; ++m) fs6_mul(it.w, m, coef(c, m).c0, coef(c, m).c1);
  return c;
}
fp12 lanes_xform(fp12 a, int xf) {
  fp12 r;
  for (int m = 0; m < 6; ++m) coef(r, m) = fs6_xform(coef(a, m), xf, m, block_consts());
  return r;
}
fp12 lanes_conj(fp12 r) {
  for (int m = 1; m < 6; m += 2) coef(r, m) = fp2{fs6_neg(coef(r, m).c0), fs6_neg(coef(r, m).c1)};
  return r;
}

// The ops of one operand pair (r, a; values below 2.3p) against the tower:
// 0, or 1 product, 2 conjugated product, 3 frob1, 4 frob2, 5 squaring,
// 6 conj; + 8 if a stored value left its bound.
int check_ops(const fp12& r, const fp12& a) {
  const fp12 rr = reduced(r), ra = reduced(a);
  item it;
  memset(&it, 0, sizeof it);
  if (!put_r(it, r) || !put_a(it, a)) return 8;
  auto stored = [&](fp12 v, uint32_t top) {
    bool ok = true;
    for (int m = 0; m < 6; ++m) ok = ok && bounded(coef(v, m).c0, top) && bounded(coef(v, m).c1, top);
    return ok;
  };
  fp12 c = lanes_mul(it);
  if (!stored(c, TOP_23P)) return 1 + 8;
  if (!equals(c, fp12_mul(rr, ra))) return 1;
  {
    // the product's outputs as the next product's R: the xi forms of a 2.3p value
    item nx = it;
    if (!put_r(nx, c)) return 1 + 8;
    const fp12 c2 = lanes_mul(nx);
    if (!stored(c2, TOP_23P)) return 1 + 8;
    if (!equals(c2, fp12_mul(fp12_mul(rr, ra), ra))) return 1;
  }
  const fp12 ca = lanes_xform(a, FS6_X_CONJ);
  if (!stored(ca, TOP_23P) || !put_a(it, ca)) return 2 + 8;
  if (!equals(lanes_mul(it), fp12_mul(rr, fp12_conj(ra)))) return 2;
  const fp12 f1 = lanes_xform(a, FS6_X_FROB1);
  if (!stored(f1, TOP_201P)) return 3 + 8;
  if (!equals(f1, fp12_frob1(ra))) return 3;
  const fp12 f2 = lanes_xform(a, FS6_X_FROB2);
  if (!stored(f2, TOP_201P)) return 4 + 8;
  if (!equals(f2, fp12_frob2(ra))) return 4;
  {
    item sq;
    memset(&sq, 0, sizeof sq);
    if (!put_r(sq, a)) return 5 + 8;  // A parked in R's slots
    fp12 s;
    for (int m = 0; m < 6; ++m) m6_sqr(sq.w, m, coef(s, m).c0, coef(s, m).c1);
    if (!stored(s, TOP_23P)) return 5 + 8;
    if (!equals(s, fp12_sqr(ra))) return 5;
  }
  const fp12 cj = lanes_conj(r);
  if (!stored(cj, TOP_23P)) return 6 + 8;  // the even coefficients stay as they are
  if (!equals(cj, fp12_conj(rr))) return 6;
  return 0;
}

// ---------------------------------------------------------------- the kernel, emulated
fp ld_word(const uint32_t* buf, size_t off) {
  fp a;
  for (int l = 0; l < FP_LIMBS; ++l) a.l[l] = buf[off + l * ENG_WAVE_WORDS];
  return a;
}
void st_word(uint32_t* buf, size_t off, const fp& a) {
  for (int l = 0; l < FP_LIMBS; ++l) buf[off + l * ENG_WAVE_WORDS] = a.l[l];
}

struct emu_out {
  std::vector<fp> R;       // [cnt][12]: the items' final R
  size_t max_word = 0;     // one past the largest word addressed in xbuf
  bool odd = false;        // a lane's word pair not 8-byte aligned
  bool stored_bad = false; // a valid item's value stored to LDS or a plane left its bound
};

// k_eng_fe_seg6(seg) over `cnt` items, its waves' 64 lanes in lockstep (every
// lane of an op reads before any lane writes), with the kernel's own address,
// schedule and arithmetic functions.  arith = false: the addresses alone.
void run_kernel(int seg, size_t cnt, size_t r0, const uint32_t* consts, uint32_t* xbuf, const uint8_t* flags, uint32_t* fb,
                uint8_t* status, emu_out& out, bool arith = true) {
  out.R.assign(cnt * 12, fp_zero());
  const size_t waves = (cnt + M6_ITEMS_PER_WAVE - 1) / M6_ITEMS_PER_WAVE;
  std::vector<uint32_t> lds(M6_ITEMS_PER_WAVE * M6_ITEM_WORDS);
  for (size_t w = 0; w < waves; ++w) {
    m6_lane L[64];
    fp re[64], im[64], nre[64], nim[64];
    for (int t = 0; t < 64; ++t) L[t] = m6_lane_id(cnt, w, t);
    auto item = [&](int t) { return lds.data() + L[t].gi * M6_ITEM_WORDS; };
    auto plane = [&](int t, int pl) {
      const size_t off = fs6_plane_off(L[t], pl);
      out.odd = out.odd || (off & 1);
      if (off + LIMB_SPAN + 2 > out.max_word) out.max_word = off + LIMB_SPAN + 2;
      return off;
    };
    auto store_all = [&]() {
      for (int t = 0; t < 64; ++t) {
        out.stored_bad = out.stored_bad || (L[t].valid && (!bounded(re[t], TOP_23P) || !bounded(im[t], TOP_23P)));
        m6_store(item(t), L[t].m, re[t], im[t]);
      }
    };
    for (int t = 0; t < 64; ++t) {
      const size_t off = plane(t, ENG_KB_PL_X0);
      if (!arith) continue;
      const fp2 x = fs6_ld_plane(xbuf + off);
      re[t] = x.c0, im[t] = x.c1;
    }
    if (arith) store_all();
    const int ns = fs6_nsteps(seg);
    for (int s = 0; s < ns; ++s) {
      const fs6_step p = fs6_plan(seg, s);
      if (p.xf == FS6_X_SQR) {
        if (arith) {
          fp2 a[64];
          for (int t = 0; t < 64; ++t) a[t] = fs6_get_a(item(t), L[t].m);
          for (int t = 0; t < 64; ++t) m6_store(item(t), L[t].m, a[t].c0, a[t].c1);
          for (int t = 0; t < 64; ++t) m6_sqr(item(t), L[t].m, a[t].c0, a[t].c1);
          for (int t = 0; t < 64; ++t) {
            out.stored_bad = out.stored_bad || (L[t].valid && (!bounded(a[t].c0, TOP_23P) || !bounded(a[t].c1, TOP_23P)));
            fs6_put_a(item(t), L[t].m, a[t]);
          }
          store_all();
        }
      } else {
        for (int t = 0; t < 64; ++t) {
          const size_t off = plane(t, p.plane);
          if (!arith) continue;
          const fp2 a = fs6_xform(fs6_ld_plane(xbuf + off), p.xf, L[t].m, consts);
          out.stored_bad = out.stored_bad || (L[t].valid && (!bounded(a.c0, TOP_23P) || !bounded(a.c1, TOP_23P)));
          fs6_put_a(item(t), L[t].m, a);
        }
      }
      if (arith) {
        for (int t = 0; t < 64; ++t) fs6_mul(item(t), L[t].m, nre[t], nim[t]);
        for (int t = 0; t < 64; ++t) {
          re[t] = nre[t], im[t] = nim[t];
          if (p.conj_r && (L[t].m & 1)) re[t] = fs6_neg(re[t]), im[t] = fs6_neg(im[t]);
        }
        store_all();
      }
      for (int t = 0; t < 64; ++t) {
        if (!L[t].valid) continue;
        for (int pl : {ENG_KB_PL_M, ENG_KB_PL_T2}) {
          if (!(pl == ENG_KB_PL_M ? p.st_m : p.st_t2)) continue;
          const size_t off = plane(t, pl);
          if (!arith) continue;
          fs6_st_plane(xbuf + off, re[t], im[t]);
          out.stored_bad = out.stored_bad || !bounded(ld_word(xbuf, off), TOP_201P) || !bounded(ld_word(xbuf, off + 1), TOP_201P);
        }
      }
    }
    if (!arith) continue;
    for (int t = 0; t < M6_ITEMS_PER_WAVE * M6_LANES; ++t) {
      if (!L[t].valid) continue;
      out.R[fs6_item(L[t]) * 12 + 2 * L[t].m] = re[t];
      out.R[fs6_item(L[t]) * 12 + 2 * L[t].m + 1] = im[t];
    }
    if (seg == FS6_LAST_SEG) {
      uint64_t vote = 0, fl = 0;
      for (int t = 0; t < 64; ++t) {
        vote |= (uint64_t)fs6_is_one(re[t], im[t], L[t].m) << t;
        fl |= (uint64_t)(L[t].valid && flags[fs6_item(L[t])]) << t;
      }
      constexpr int HALF = ENG_ROUNDS_PER_BLOCK * M6_LANES;
      for (int t = 0; t < 64; ++t) {
        const bool all = ((vote >> (M6_LANES * L[t].gi)) & 0x3Full) == 0x3Full;
        const size_t i = fs6_item(L[t]);
        const bool flagged = L[t].valid && flags[i];
        if (L[t].valid && L[t].m == 0 && !all && !flagged && status[r0 + i] == ST_OK) status[r0 + i] = ST_PAIRING;
        if (t == 0 && (fl & ((1ull << HALF) - 1)) != 0) fb[1 + fb[0]++] = (uint32_t)L[t].blk;
        if (t == HALF && (fl >> HALF) != 0) fb[1 + fb[0]++] = (uint32_t)L[t].blk;
      }
    }
  }
}

// Seeded planes; plane T holds an element of the cyclotomic subgroup, as in
// the FE (E_CYCA, the 12-lane side's squaring of t, is the cyclotomic one).
void fill_planes(std::vector<uint32_t>& xbuf, size_t cnt, rng& g, const uint8_t* ones) {
  for (size_t i = 0; i < cnt; ++i)
    for (int pl = 0; pl < ENG_KB_PLANES; ++pl) {
      fp12 v = g.next12();
      if (pl == ENG_KB_PL_T) {
        v = fp12_mul(fp12_conj(v), fp12_inv(v));
        v = fp12_mul(fp12_frob2(v), v);
      }
      for (int k = 0; k < 12; ++k) {
        const fp c = (k & 1) ? coef(v, k / 2).c1 : coef(v, k / 2).c0;
        st_word(xbuf.data(), kb_off(i, pl, k), ones && ones[i] ? (k == 0 ? fp_one() : fp_zero()) : c);
      }
    }
}
}  // namespace

extern "C" {

// n seeded operand pairs (values CI): the number of failing pairs; *first = check_ops' code of the first.
int fs6_random(int n, uint64_t seed, int* first) {
  rng g{seed | 1};
  int bad = 0;
  *first = 0;
  for (int t = 0; t < n; ++t) {
    const fp12 r = g.next12(), a = g.next12();
    const int rc = check_ops(r, a);
    if (rc && !bad) *first = rc;
    bad += rc != 0;
  }
  return bad;
}

// Operands at the limb maxima of a stored value (every limb 2^28 - 1 under the
// top limb of 2.3p), in R and in A:
//   0  re = im = maximum (re + im at its bound)
//   1  re = maximum, im = 0 (re - im + 8p at its bound, 10.3p: the wrapped terms' operand)
//   2  re = 0, im = maximum (its mirror)
// 0, or 100 * (1 + case) + check_ops' code.
int fs6_edge() {
  fp mx;
  for (int i = 0; i < FP_LIMBS; ++i) mx.l[i] = FP_MASK;
  mx.l[FP_LIMBS - 1] = TOP_23P - 1;
  const fp z = fp_zero();
  const fp2 pat[3] = {fp2{mx, mx}, fp2{mx, z}, fp2{z, mx}};
  for (int cr = 0; cr < 3; ++cr)
    for (int ca = 0; ca < 3; ++ca) {
      fp12 r, a;
      for (int k = 0; k < 6; ++k) coef(r, k) = pat[cr], coef(a, k) = pat[ca];
      const int rc = check_ops(r, a);
      if (rc) return 100 * (1 + 3 * cr + ca) + rc;
    }
  return 0;
}

// Segment `seg` (1..5) over `cnt` items on seeded planes (items with ones[i]
// hold the Fp12 one in every plane, so their R is 1), through the emulated
// kernel and, item by item, through hostsim's emulation of the same
// ENG_PROG_FEK segment: planes M, T, T2 and R must be equal as residues, the
// other planes unchanged, every stored value within its bound.  status_io
// (cnt bytes at r0 = 0) and fb_out (1 + eng_blocks(cnt) words) are the
// kernel's; for the last segment the verdicts must be those of the 12-lane
// R for valid, unflagged items with ST_OK and untouched elsewhere.
// 0, or 1000 * (1 + item) + 1 planes, 2 R, 3 verdict; -1 a bound, -2 an address.
int fs6_segment(int seg, int cnt, uint64_t seed, const uint8_t* ones, const uint8_t* flags, uint8_t* status_io,
                uint32_t* fb_out) {
  rng g{seed | 1};
  const size_t words = eng_blk_words(eng_blocks((size_t)cnt), ENG_KB_PLANES);
  std::vector<uint32_t> xbuf(words, 0xEEEEEEEEu);
  fill_planes(xbuf, (size_t)cnt, g, ones);
  const std::vector<uint32_t> before = xbuf;
  const std::vector<uint8_t> st0(status_io, status_io + cnt);
  fb_out[0] = 0;
  emu_out out;
  run_kernel(seg, (size_t)cnt, 0, block_consts(), xbuf.data(), flags, fb_out, status_io, out);
  if (out.stored_bad) return -1;
  if (out.max_word > words || out.odd) return -2;
  // rounds past cnt in the last block stay unwritten
  for (size_t i = (size_t)cnt; i < eng_blocks((size_t)cnt) * ENG_ROUNDS_PER_BLOCK; ++i)
    for (int pl = 0; pl < ENG_KB_PLANES; ++pl)
      if (xbuf[kb_off(i, pl, 0)] != 0xEEEEEEEEu) return -2;
  for (int i = 0; i < cnt; ++i) {
    static HostGroup G;
    G = HostGroup();
    host_scramble(G, 0x9E3779B97F4A7C15ull + (uint64_t)i);
    host_consts(G, g1a{fp_zero(), fp_zero()});
    for (int pl = 0; pl < ENG_KB_PLANES; ++pl)
      for (int k = 0; k < 12; ++k) G.fbuf[12 * pl + k] = ld_word(before.data(), kb_off((size_t)i, pl, k));
    host_exec(G, ENG_PROG_FEK + ENG_PROG_FEK_OFF[seg], ENG_PROG_FEK_OFF[seg + 1] - ENG_PROG_FEK_OFF[seg]);
    for (int pl = 0; pl < ENG_KB_PLANES; ++pl)
      for (int k = 0; k < 12; ++k) {
        const fp got = ld_word(xbuf.data(), kb_off((size_t)i, pl, k));
        if (!bounded(got, TOP_201P) || !same(got, G.fbuf[12 * pl + k])) return 1000 * (1 + i) + 1;
      }
    bool one = true;
    for (int k = 0; k < 12; ++k) {
      if (!same(out.R[(size_t)i * 12 + k], G.get(ENG_E_R + k))) return 1000 * (1 + i) + 2;
      one = one && same(G.get(ENG_E_R + k), k == 0 ? fp_one() : fp_zero());
    }
    const uint8_t want = seg == FS6_LAST_SEG && !one && !flags[i] && st0[i] == ST_OK ? (uint8_t)ST_PAIRING : st0[i];
    if (status_io[i] != want) return 1000 * (1 + i) + 3;
  }
  return 0;
}

// The addresses of k_eng_fe_seg6 over all five segments for `cnt` items,
// without the arithmetic: one past the largest word its lanes address in the
// state planes (out[0]), the planes' size eng_blk_words(eng_blocks(cnt),
// ENG_KB_PLANES) (out[1]); out[2] = 1 if some lane's two words are not 8-byte
// aligned.
void fs6_extents(uint64_t cnt, uint64_t* o) {
  emu_out out;
  size_t mx = 0;
  for (int seg = 1; seg <= FS6_LAST_SEG; ++seg) {
    run_kernel(seg, cnt, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out, false);
    mx = out.max_word > mx ? out.max_word : mx;
  }
  o[0] = mx, o[1] = eng_blk_words(eng_blocks(cnt), ENG_KB_PLANES), o[2] = out.odd;
}
}

#ifdef FS6_MAIN
int main() {
  int first = 0;
  const int bad = fs6_random(64, 7, &first);
  const int edge = fs6_edge();
  printf("fs6_random: %d bad (first %d), edge %d\n", bad, first, edge);
  int segs = 0;
  for (int seg = 1; seg <= FS6_LAST_SEG; ++seg) {
    const int cnt = 11;
    uint8_t ones[cnt] = {0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0}, flags[cnt] = {0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0}, st[cnt] = {0};
    st[3] = ST_SUBGROUP;
    uint32_t fb[1 + 3];
    const int rc = fs6_segment(seg, cnt, 20 + seg, ones, flags, st, fb);
    printf("fs6_segment %d: %d (fb %u)\n", seg, rc, fb[0]);
    segs += rc != 0 || (seg == FS6_LAST_SEG ? fb[0] != 2 : fb[0] != 0);
  }
  int ext = 0;
  for (uint64_t cnt : {1, 4, 5, 6, 9, 10, 11, 14, 15, 16, 63, 64, 65}) {
    uint64_t o[3];
    fs6_extents(cnt, o);
    ext += o[0] > o[1] || o[2];
  }
  printf("fs6_extents: %d bad\n", ext);
  return bad || edge || segs || ext;
}
#endif
