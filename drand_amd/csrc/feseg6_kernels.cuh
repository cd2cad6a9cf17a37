// Segments 1..5 of the Karabina FE with one Fp2 coefficient per lane
// (feseg6.cuh):
//
//   k_eng_fe_seg6   6 lanes per item, 10 items per wave: two consecutive
//                   5-round blocks of the state planes
//
// It computes what k_eng_fe_seg(e) computes for e = 1..5 (pairing_engine.cuh):
// the same planes in and out, the same verdicts and fallback list after the
// last one.  Segment 0 (the easy part, with its inversion) and k_eng_fe_fb stay
// on the 12-lane engine.  Written by hand: no interpreter, no generated tables.
#pragma once
#include "feseg6.cuh"
#include "pairing_engine.cuh"

namespace dgpu {

// Grid: one wave per M6_ITEMS_PER_WAVE items (addresses: miller6.cuh m6_lane_id).
// seg == 5: R == 1 -> verdict for valid, unflagged items; each of the wave's
// two blocks joins the fallback list fb = [count, blocks...] (k_eng_fe_fb's
// units) once if any of its items is flagged.  Flagged items hold no f0 / f3:
// their products are garbage and reach no verdict.
__global__ void __launch_bounds__(ENG_BLOCK, 2) k_eng_fe_seg6(int seg, size_t cnt, size_t r0,
                                                           const uint32_t* __restrict__ consts,
                                                           uint32_t* __restrict__ xbuf,
                                                           const uint8_t* __restrict__ flags, uint32_t* __restrict__ fb,
                                                           uint8_t* __restrict__ status) {
  __shared__ uint32_t lds[M6_ITEMS_PER_WAVE * M6_ITEM_WORDS];
  const int lane = threadIdx.x & 63;
  const m6_lane L = m6_lane_id(cnt, blockIdx.x, lane);
  const int m = L.m;
  uint32_t* it = lds + L.gi * M6_ITEM_WORDS;
  fp re, im;
  {
    const fp2 x = fs6_ld_plane(xbuf + fs6_plane_off(L, ENG_KB_PL_X0));
    re = x.c0, im = x.c1;
  }
  m6_store(it, m, re, im);
  asm volatile("" ::: "memory");
  // every lane's reads of an op issue before its writes, and one wave's LDS
  // queue is in order (engine.cuh eng_sync): compiler fences order the ops
  const int ns = fs6_nsteps(seg);
#pragma unroll 1
  for (int s = 0; s < ns; ++s) {
    const fs6_step p = fs6_plan(seg, s);
    if (p.xf == FS6_X_SQR) {
      // A <- A^2: A takes R's slots for m6_sqr while R_m waits in (re, im)
      const fp2 t = fs6_get_a(it, m);
      m6_store(it, m, t.c0, t.c1);
      asm volatile("" ::: "memory");
      fp2 sq;
      m6_sqr(it, m, sq.c0, sq.c1);
      asm volatile("" ::: "memory");
      fs6_put_a(it, m, sq);
      m6_store(it, m, re, im);
    } else {
      fs6_put_a(it, m, fs6_xform(fs6_ld_plane(xbuf + fs6_plane_off(L, p.plane)), p.xf, m, consts));
    }
    asm volatile("" ::: "memory");
    fs6_mul(it, m, re, im);
    asm volatile("" ::: "memory");
    if (p.conj_r && (m & 1)) re = fs6_neg(re), im = fs6_neg(im);
    m6_store(it, m, re, im);
    asm volatile("" ::: "memory");
    if (L.valid) {
      if (p.st_m) fs6_st_plane(xbuf + fs6_plane_off(L, ENG_KB_PL_M), re, im);
      if (p.st_t2) fs6_st_plane(xbuf + fs6_plane_off(L, ENG_KB_PL_T2), re, im);
    }
  }
  if (seg == FS6_LAST_SEG) {
    const uint64_t vote = __ballot(fs6_is_one(re, im, m));
    const bool all = ((vote >> (M6_LANES * L.gi)) & 0x3Full) == 0x3Full;
    const size_t i = fs6_item(L);
    const bool flagged = L.valid && flags[i];
    if (L.valid && m == 0 && !all && !flagged && status[r0 + i] == ST_OK) status[r0 + i] = ST_PAIRING;
    const uint64_t fl = __ballot(flagged);
    constexpr int HALF = ENG_ROUNDS_PER_BLOCK * M6_LANES;  // the wave's second block starts at this lane
    if (lane == 0 && (fl & ((1ull << HALF) - 1)) != 0) fb[1 + atomicAdd(fb, 1u)] = (uint32_t)L.blk;
    if (lane == HALF && (fl >> HALF) != 0) fb[1 + atomicAdd(fb, 1u)] = (uint32_t)L.blk;
  }
}

}  // namespace dgpu
