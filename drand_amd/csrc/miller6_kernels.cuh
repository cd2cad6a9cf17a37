// The Miller product f = prod of lines with one Fp2 coefficient per lane
// (miller6.cuh), and the norm tail that follows it:
//
//   k_eng_miller6      6 lanes per item, 10 items per wave: two consecutive
//                      5-round blocks of the line buffer; f -> fbuf plane 0
//   k_eng_miller_tail  N1 = Norm(f): the last ENG_MILLER_TAIL_OPS ops of
//                      ENG_PROG_MILLER on the 12-lane engine, f from fbuf
//
// Together they compute what k_eng_miller computes (pairing_engine.cuh): the
// same line buffer in, the same fbuf plane and n1 out.  Written by hand: no
// interpreter, no generated tables.
#pragma once
#include "miller6.cuh"
#include "pairing_engine.cuh"

namespace dgpu {

static_assert(M6_ITEMS_PER_WAVE * M6_ITEM_WORDS * 4 * 8 <= 160 * 1024, "two waves per SIMD fit the CU's 160 KiB of LDS");

// Grid: one wave per M6_ITEMS_PER_WAVE items (addresses: miller6.cuh m6_lane_id).
__global__ void __launch_bounds__(ENG_BLOCK, 2) k_eng_miller6(size_t cnt, const uint32_t* __restrict__ lines,
                                                           uint32_t* __restrict__ fbuf) {
  __shared__ uint32_t lds[M6_ITEMS_PER_WAVE * M6_ITEM_WORDS];
  const m6_lane L = m6_lane_id(cnt, blockIdx.x, threadIdx.x & 63);
  const int m = L.m;
  uint32_t* it = lds + L.gi * M6_ITEM_WORDS;
  m6_store(it, m, m == 0 ? fp_one() : fp_zero(), fp_zero());
  asm volatile("" ::: "memory");
  const uint32_t* lp = lines + m6_line_off(L, 0);
  uint32_t* lslot = it + (M6_L1 + 2 * m) * ENG_SLOT_WORDS;
  // every lane's reads of an op issue before its writes, and one wave's LDS
  // queue is in order (engine.cuh eng_sync): compiler fences order the ops
  m6_sched sc;
#pragma unroll 1
  for (int step = 0; step < ENG_LINE_STEPS; ++step) {
    fp re, im;
    if (m6_sched_sqr(sc)) {
      m6_sqr(it, m, re, im);
      asm volatile("" ::: "memory");
      m6_store(it, m, re, im);
      asm volatile("" ::: "memory");
    }
    {
      const uint32_t* p = lp + (size_t)step * FP_LIMBS * ENG_WAVE_WORDS;  // m6_line_off(L, step)
#pragma unroll
      for (int l = 0; l < FP_LIMBS; ++l) {
        const uint2 v = *reinterpret_cast<const uint2*>(p + l * ENG_WAVE_WORDS);
        re.l[l] = v.x, im.l[l] = v.y;
      }
      eng_st(lslot, re);
      eng_st(lslot + ENG_SLOT_WORDS, im);
      asm volatile("" ::: "memory");
    }
#pragma unroll 1
    for (int line = M6_L1; line <= M6_L2; line += M6_L2 - M6_L1) {
      m6_line_mul(it, m, line, re, im);
      asm volatile("" ::: "memory");
      m6_store(it, m, re, im);
      asm volatile("" ::: "memory");
    }
    m6_sched_next(sc);
  }
  if (L.valid) {
    // the loop's values are below 2.3p (miller6.cuh); fbuf's readers expect slot values, below 2.01p
    const fp fre = eng_reduce(eng_ld(it + m * M6_COEF_WORDS)), fim = eng_reduce(eng_ld(it + m * M6_COEF_WORDS + ENG_SLOT_WORDS));
    uint32_t* fo = fbuf + m6_f_off(L);
#pragma unroll
    for (int l = 0; l < FP_LIMBS; ++l) *reinterpret_cast<uint2*>(fo + l * ENG_WAVE_WORDS) = make_uint2(fre.l[l], fim.l[l]);
  }
}

// N1 = Norm(f) of the f that k_eng_miller6 left in fbuf's plane 0 (loaded as
// k_eng_fe_seg loads it); f stays where it is.
__global__ void __launch_bounds__(ENG_BLOCK, 3) k_eng_miller_tail(size_t cnt, const uint32_t* __restrict__ consts,
                                                               uint32_t* __restrict__ fbuf, uint32_t* __restrict__ n1) {
  __shared__ uint32_t lds[ENG_LDS_SLOTS_MILLER * ENG_SLOT_WORDS];
  uint32_t* c = lds;
  eng_load_consts(c, consts);
  const eng_lane L = eng_lane_id(cnt);
  uint32_t* g = lds + ENG_GBASE_MILLER[L.g] * ENG_SLOT_WORDS;
  eng_st(g + (ENG_M_F + L.k) * ENG_SLOT_WORDS, ld_blk(fbuf, eng_blk_off(L.blk, ENG_F_PLANES, 0, L.g, L.k)));
  asm volatile("" ::: "memory");
  eng_exec<false, false, 1>(ENG_PROG_MILLER + ENG_PROG_MILLER_LEN - ENG_MILLER_TAIL_OPS, ENG_MILLER_TAIL_OPS, g, c, L,
                            eng_io{nullptr, fbuf, n1, cnt});
}

}  // namespace dgpu
