// Index functions of the pairing engine's HBM buffers and, beside each, the
// extent it implies: what the kernels address and what the host allocates are
// read off the same lines.  Host and device functions, no kernels: a host-only
// program (tests/scratch_layout_check.hip) includes this header alone.
#pragma once
#include "engine.cuh"
#include "kernels.cuh"

namespace dgpu {

constexpr int ENG_ROUNDS_PER_BLOCK = ENG_GROUPS_PER_WAVE;      // one wave: 5 rounds
constexpr int ENG_LINE_STEPS = 68;

// Wave-blocked layout of the line and f buffers: block b (rounds 5b..5b+4)
// owns planes [b][plane][limb][60] with word g*12 + e (group g, export e), so
// every limb access of a wave is one contiguous 240-byte segment (a
// round-fastest SoA would scatter the 60 lanes over 12 planes, 20 bytes each).
constexpr int ENG_WAVE_WORDS = ENG_GROUPS_PER_WAVE * 12;
DG_FN size_t eng_blk_off(size_t blk, int planes, int plane, int g, int e) {
  return (blk * planes + plane) * FP_LIMBS * ENG_WAVE_WORDS + g * 12 + e;
}
// words of `blocks` whole blocks of `planes` planes: past every
// eng_blk_off(blk < blocks, planes, plane < planes, g < 5, e < 12) + limb * ENG_WAVE_WORDS
DG_FN constexpr size_t eng_blk_words(size_t blocks, int planes) { return blocks * planes * FP_LIMBS * ENG_WAVE_WORDS; }
DG_FN constexpr size_t eng_blocks(size_t rounds) { return (rounds + ENG_ROUNDS_PER_BLOCK - 1) / ENG_ROUNDS_PER_BLOCK; }
// the f buffer's planes (f / t, then t2)
constexpr int ENG_F_PLANES = 2;
// N1 and its like, [limb][i] over the chunk's rounds (st_soa / ld_soa with stride cnt <= rounds)
DG_FN constexpr size_t eng_n1_words(size_t rounds) { return rounds * FP_LIMBS; }

// Karabina FE state planes (gen_engine.py PL_*: t, t2, the exponentiation
// input m, the six stored m^(2^s)) in fbuf's wave-blocked layout with
// ENG_KB_PLANES planes: [block of 5 rounds][plane][limb][g * 12 + component];
// eng_blk_words(eng_blocks(rounds), ENG_KB_PLANES) words.
DG_FN size_t kb_off(size_t i, int plane, int comp) {
  const size_t blk = i / ENG_ROUNDS_PER_BLOCK;
  const int g = (int)(i - blk * ENG_ROUNDS_PER_BLOCK);
  return (blk * ENG_KB_PLANES + plane) * FP_LIMBS * ENG_WAVE_WORDS + g * 12 + comp;
}

// Scratch planes of the small-batch cofactor clearing (pairing_engine.cuh
// k_cof_*), SoA with stride n: plane set X starts COF_X * n words into the
// buffer and COF_WORDS * n words hold them all.
//   pj [6 fp] | pa [4] | psia [4] | t1 [12] | t0a [4] | t2 [12] | u [6]
constexpr int COF_PJ = 0;
constexpr int COF_PA = COF_PJ + G2J_WORDS;
constexpr int COF_PSIA = COF_PA + G2A_WORDS;
constexpr int COF_T1 = COF_PSIA + G2A_WORDS;
constexpr int COF_T_WORDS = 12 * FP_WORDS;  // k_eng_lines' t_out: T of both pairs, homogeneous
constexpr int COF_T0A = COF_T1 + COF_T_WORDS;
constexpr int COF_T2 = COF_T0A + G2A_WORDS;
constexpr int COF_U = COF_T2 + COF_T_WORDS;
constexpr int COF_WORDS = COF_U + G2J_WORDS;

}  // namespace dgpu
