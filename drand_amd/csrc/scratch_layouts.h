// The layout of every device scratch buffer that holds more than one region
// (scratch_carve.h: one fill() per buffer gives its size and its pointers).
// Grouped by the code that owns the buffer; capi.hip's carve() applies them.
// Host code; it takes the kernels' own sizes and index functions from their
// headers, which a host-only program includes under DG_NO_KERNELS.
// Which program checks which layout: tests/scratch_layout_check.hip every
// layout here except those of the row ingest group; tests/check_rows_check.cpp
// that group (ingest_rows_layout, check_rows_layout, check_lists_layout);
// tests/keyed_groups_check.cpp the keyed calls' RLC scratch (keyed_rlc_layout;
// keyed_table_layout and keyed_exact_layout are plain arrays back to back).
//
// Alignment: a region is aligned to the widest access its kernels make --
// 16 bytes for k_h2c_finish's park quads, 8 for the wave-blocked planes
// (uint2) and 64-bit arrays, 4 for word arrays.  No layout below needs
// padding for it; the check program asserts that.
#pragma once
#include "engine_layout.cuh"
#include "recover.cuh"
#include "rlc_msm.cuh"
#include "scratch_carve.h"
#include "check_rows.cuh"  // (behind the headers that bring the HIP runtime's function qualifiers)

namespace dgpu {

// ---------------------------------------------------------------- pairing engine
// Karabina FE state of one chunk of `blocks` whole 5-round blocks (capacity
// capb = 5 * blocks rounds; the r03i fault, DESIGN.md 2b': the planes are
// addressed by kb_off over whole blocks, so every region is sized by capb,
// never by the chunk's round count).
struct eng_kb_layout {
  uint32_t* xbuf;  // the state planes: eng_blk_words(blocks, ENG_KB_PLANES), kb_off
  uint32_t* pbuf;  // product of the six norms, [limb][capb]
  uint32_t* pre;   // its prefix products (k_eng_inv)
  uint32_t* ebuf;  // the six excluded products, [snap][limb][capb]
  uint32_t* fb;    // the fallback list [count, blocks...]
  uint8_t* flags;  // per round
  void fill(carver& c, size_t blocks) {
    const size_t capb = blocks * ENG_ROUNDS_PER_BLOCK;
    xbuf = c.take<uint32_t>(eng_blk_words(blocks, ENG_KB_PLANES), 8);
    pbuf = c.take<uint32_t>(eng_n1_words(capb));
    pre = c.take<uint32_t>(eng_n1_words(capb));
    ebuf = c.take<uint32_t>(ENG_KB_NSNAP * eng_n1_words(capb));
    fb = c.take<uint32_t>(capb);
    flags = c.take<uint8_t>(capb);
  }
};

// Engine bytes per round and lane (line buffer + f planes + N1 + Karabina
// state): one block of each, over its five rounds.
inline size_t eng_bytes_per_round() {
  return ((eng_blk_words(1, ENG_LINE_STEPS) + eng_blk_words(1, ENG_F_PLANES) + eng_n1_words(ENG_ROUNDS_PER_BLOCK)) * 4 +
          layout_bytes<eng_kb_layout>((size_t)1)) /
         ENG_ROUNDS_PER_BLOCK;
}

// k_eng_inv's prefix products ([limb][cap], cap <= 5 * blocks) reuse the line
// buffer of the chunk: they fit in any whole number of blocks.
static_assert(eng_n1_words(ENG_ROUNDS_PER_BLOCK) <= eng_blk_words(1, ENG_LINE_STEPS),
              "the prefix products of a block's rounds fit in its line planes");

// ---------------------------------------------------------------- G2 hash
// h_tmp of n rounds: the field elements u, the two SSWU points q, and (the
// per-round path) k_h2c_finish's park region in whole 64-round blocks and its
// redo flags.  The RLC points take u and q alone.
struct h2c_tmp_layout {
  uint32_t* u;     // [4 fp][limb][n]
  uint32_t* q;     // Q0, Q1 Jacobian: [2][6 fp][limb][n]
  uint32_t* park;  // h2c_park_word; 16-byte quads
  uint8_t* redo;
  void fill(carver& c, size_t n, bool finish) {
    u = c.take<uint32_t>(4 * FP_WORDS * n);
    q = c.take<uint32_t>(2 * G2J_WORDS * n);
    park = finish ? c.take<uint32_t>(h2c_park_words(n), 16) : nullptr;
    redo = finish ? c.take<uint8_t>(n) : nullptr;
  }
};

// cof_tmp: the planes of the small-batch cofactor clearing.  The k_cof_*
// kernels take the base and address plane set X at COF_X * n.
struct cof_tmp_layout {
  uint32_t *pj, *pa, *psia, *t1, *t0a, *t2, *u;
  void fill(carver& c, size_t n) {
    pj = c.take<uint32_t>(G2J_WORDS * n);
    pa = c.take<uint32_t>(G2A_WORDS * n);
    psia = c.take<uint32_t>(G2A_WORDS * n);
    t1 = c.take<uint32_t>(COF_T_WORDS * n);
    t0a = c.take<uint32_t>(G2A_WORDS * n);
    t2 = c.take<uint32_t>(COF_T_WORDS * n);
    u = c.take<uint32_t>(G2J_WORDS * n);
  }
};

// ---------------------------------------------------------------- RLC
// The levels of a pairwise sum tree over n leaves of jw-word Jacobian points,
// for two point sets P and S: level l has sz[l] nodes (sz[0] = n, halved
// rounding up to the single root), P[l] then S[l], SoA with stride sz[l].
struct sum_levels {
  static constexpr int MAX_LEVELS = 65;
  int levels;
  size_t sz[MAX_LEVELS];
  uint32_t *P[MAX_LEVELS], *S[MAX_LEVELS];
  int top() const { return levels - 1; }
  void fill(carver& c, size_t n, int jw) {
    levels = 0;
    for (size_t v = n;; v = (v + 1) / 2) {
      sz[levels] = v;
      P[levels] = c.take<uint32_t>(v * jw);
      S[levels] = c.take<uint32_t>(v * jw);
      ++levels;
      if (v <= 1) break;
    }
  }
};

// rlc_tree: the segment trees' levels, then the batch's points R_i as a
// Jacobian SoA whose X, Y planes (aw words) are the affine points once
// k_g*_batch_affine has run over the Z planes behind them.
struct rlc_tree_layout {
  sum_levels T;
  uint32_t* rpts;  // R_i: X, Y
  uint32_t* rz;    // R_i: Z
  void fill(carver& c, size_t n, int aw, int jw) {
    T.fill(c, n, jw);
    rpts = c.take<uint32_t>(n * aw);
    rz = c.take<uint32_t>(n * (jw - aw));
  }
};

// A root: P then S, stride-1 Jacobian points of the signature group (also the
// wire format of dgpu_rlc_root_device and of the devices' all-gather).
struct rlc_root_layout {
  uint32_t *P, *S;
  void fill(carver& c, int jw) {
    P = c.take<uint32_t>(jw);
    S = c.take<uint32_t>(jw);
  }
};

// rlc_conf: the confirmation root, the compaction counter, the list of the mc
// candidates that failed.
struct rlc_conf_layout {
  rlc_root_layout root;
  uint32_t *count, *list;
  void fill(carver& c, size_t mc, int jw) {
    root.fill(c, jw);
    count = c.take<uint32_t>(1);
    list = c.take<uint32_t>(mc);
  }
};

// The bucket MSM's small buffers (rlc_msm.cuh).
struct msm_counts_layout {
  uint32_t *counts, *offsets, *cursor;
  void fill(carver& c) {
    counts = c.take<uint32_t>(MSM_KEYS);
    offsets = c.take<uint32_t>(MSM_KEYS);
    cursor = c.take<uint32_t>(MSM_KEYS);
  }
};
struct msm_list_layout {
  uint32_t *list, *keys;  // MSM_MW entries per round; the key of every entry
  uint32_t* spare;        // one word past the keys, kept from the first sizing
  void fill(carver& c, size_t n) {
    list = c.take<uint32_t>(MSM_MW * n);
    keys = c.take<uint32_t>(MSM_MW * n);
    spare = c.take<uint32_t>(1);
  }
};
struct msm_runs_layout {
  uint32_t *runs, *runs2;  // the window sums and their ping-pong partner
  void fill(carver& c, int jw) {
    runs = c.take<uint32_t>((size_t)MSM_MW * MSM_RUNS * jw);
    runs2 = c.take<uint32_t>((size_t)MSM_MW * MSM_RUNS * jw);
  }
};

// ---------------------------------------------------------------- misc: the data tools' small arenas
// decode_g1_key_locked: the host reads out and rc in one copy (they stay adjacent)
struct g1_key_misc {
  uint8_t* in;    // 48 B used
  uint32_t* out;  // (-x, y)
  int* rc;
  void fill(carver& c) {
    in = c.take<uint8_t>(64);
    out = c.take<uint32_t>(2 * FP_LIMBS);
    rc = c.take<int>(20);
  }
};
// decode_g2_key_locked: four 1 KiB slots
struct g2_key_misc {
  uint32_t* pk;  // affine G2, stride 1 (224 B used)
  uint32_t* g2;  // the generator, stride 1
  int* rc;
  uint8_t* in;   // 96 B used
  void fill(carver& c) {
    pk = c.take<uint32_t>(256);
    g2 = c.take<uint32_t>(256);
    rc = c.take<int>(256);
    in = c.take<uint8_t>(1024);
  }
};
// dgpu_decode_pubkey
struct pubkey_misc {
  uint8_t* in;   // <= 96 B used
  uint32_t* pt;  // stride-1 affine point (<= 224 B used)
  int* rc;
  uint8_t* xy;   // <= 192 B used
  void fill(carver& c) {
    in = c.take<uint8_t>(128);
    pt = c.take<uint32_t>(96);
    rc = c.take<int>(128);
    xy = c.take<uint8_t>(3072);
  }
};
// dgpu_decode_g1_points
struct g1_points_misc {
  int* rc;
  uint8_t* xy;
  void fill(carver& c, size_t n) {
    rc = c.take<int>(n);
    xy = c.take<uint8_t>(96 * n);
  }
};
// decode_commits_locked: t commitments of cb bytes (48 or 96), their decode codes
struct commits_misc {
  uint8_t* in;
  int* rc;
  void fill(carver& c, size_t t, size_t cb) {
    in = c.take<uint8_t>(t * cb);
    rc = c.take<int>(t);
  }
};

// ky_tab (dgpu_verify_keyed): the call's n_keys table keys decoded -- affine
// points, SoA with stride n_keys, G1 (x, y) for 48-byte keys and G2 for
// 96-byte keys --, their decode codes, and the compressed bytes as given.
struct keyed_table_layout {
  uint32_t* pts;
  int* rc;
  uint8_t* in;
  void fill(carver& c, size_t n_keys, size_t key_len) {
    pts = c.take<uint32_t>(n_keys * (key_len == 96 ? (size_t)G2A_WORDS : 2 * (size_t)FP_LIMBS));
    rc = c.take<int>(n_keys);
    in = c.take<uint8_t>(n_keys * key_len);
  }
};

// ky_rlc (dgpu_verify_keyed, RLC mode; keyed.cuh, keyed_groups.h): n records
// under n_groups keys, T list ranges, m candidate slots; aw / jw words per
// affine / Jacobian point of the signature group, kw words per key.
struct keyed_rlc_layout {
  uint32_t *counts, *offsets, *cursor, *cpos;  // [n_groups]
  uint32_t* totals;                            // listed records, non-empty groups
  uint32_t* nfail;                             // records listed for the exact check
  uint32_t *list, *lkey, *flist;               // [n]
  uint32_t *leaf_p, *leaf_s;                   // Jacobian SoA, stride n
  uint32_t* sums;                              // [P | S], Jacobian SoA of stride n_groups each
  uint32_t* part;                              // [P | S], each [A | B] of stride 2 T
  uint32_t *ch, *cs, *ckeys;                   // the candidates: affine P, S and the key, stride m (each cleared on its own)
  uint8_t* cst;                                // [m]
  void fill(carver& c, size_t n, size_t n_groups, size_t T, size_t m, int aw, int jw, int kw) {
    counts = c.take<uint32_t>(n_groups);
    offsets = c.take<uint32_t>(n_groups);
    cursor = c.take<uint32_t>(n_groups);
    cpos = c.take<uint32_t>(n_groups);
    totals = c.take<uint32_t>(2);
    nfail = c.take<uint32_t>(1);
    list = c.take<uint32_t>(n);
    lkey = c.take<uint32_t>(n);
    flist = c.take<uint32_t>(n);
    leaf_p = c.take<uint32_t>(n * jw);
    leaf_s = c.take<uint32_t>(n * jw);
    sums = c.take<uint32_t>(2 * n_groups * jw);
    part = c.take<uint32_t>(4 * T * jw);
    ch = c.take<uint32_t>(m * aw);
    cs = c.take<uint32_t>(m * aw);
    ckeys = c.take<uint32_t>(m * kw);
    cst = c.take<uint8_t>(m);
  }
};
// ky_exact: the compact batch of the mf records of failing keys
struct keyed_exact_layout {
  uint32_t *h, *s, *keys;
  uint8_t* st;
  void fill(carver& c, size_t mf, int aw, int kw) {
    h = c.take<uint32_t>(mf * aw);
    s = c.take<uint32_t>(mf * aw);
    keys = c.take<uint32_t>(mf * kw);
    st = c.take<uint8_t>(mf);
  }
};

// ---------------------------------------------------------------- row ingest
// in_rows (dgpu_verify_rows): a call's stored rows packed back to back, then
// each row's position in that run and its length -- k_ingest_rows' inputs.
// The packed run starts on a 16-byte line (the kernel's 16-byte loads are
// aligned by address, whatever a row's position).
struct ingest_rows_layout {
  uint8_t* bytes;  // [packed_bytes]
  uint64_t* off;   // [n]
  uint32_t* len;   // [n]
  void fill(carver& c, size_t packed_bytes, size_t n) {
    bytes = c.take<uint8_t>(packed_bytes, 16);
    off = c.take<uint64_t>(n);
    len = c.take<uint32_t>(n);
  }
};

// chk (dgpu_faulty_rounds_device): the scratch of the faulty list over `count`
// visited positions -- the two block-count arrays k_check_scan turns into
// block offsets, the position -> row map, the outcome flags.
struct check_rows_layout {
  uint64_t *blk_faulty, *blk_left;  // [check_blocks(count)]
  uint32_t* map;                    // [count], CHECK_NO_ROW where no row has the key
  uint8_t* flags;                   // [count], CHECK_*
  void fill(carver& c, size_t count) {
    blk_faulty = c.take<uint64_t>(check_blocks(count));
    blk_left = c.take<uint64_t>(check_blocks(count));
    map = c.take<uint32_t>(count);
    flags = c.take<uint8_t>(count);
  }
};
// chk_out (dgpu_check_rows): the two totals, then the lists at their caps
struct check_lists_layout {
  uint64_t *counts, *faulty_pos, *faulty_val, *left_rows;
  void fill(carver& c, size_t faulty_cap, size_t left_cap) {
    counts = c.take<uint64_t>(2);
    faulty_pos = c.take<uint64_t>(faulty_cap);
    faulty_val = c.take<uint64_t>(faulty_cap);
    left_rows = c.take<uint64_t>(left_cap);
  }
};

// ---------------------------------------------------------------- recovery
// rec_sel: the t selected items of a round, then their indices
struct rec_sel_layout {
  uint32_t *sel, *xs;  // [round][RECOVER_MAX_T]
  void fill(carver& c, size_t n_rounds) {
    sel = c.take<uint32_t>(n_rounds * RECOVER_MAX_T);
    xs = c.take<uint32_t>(n_rounds * RECOVER_MAX_T);
  }
};
// rec_sel of a wide group (recover_wide.cuh, t > RECOVER_MAX_T): the same two
// regions at stride t
struct rec_sel_wide_layout {
  uint32_t *sel, *xs;  // [round][t]
  void fill(carver& c, size_t n_rounds, size_t t) {
    sel = c.take<uint32_t>(n_rounds * t);
    xs = c.take<uint32_t>(n_rounds * t);
  }
};
// rec_wide_tab: the window tables of one chunk of `rounds` rounds of a wide
// group -- 8 entries per term, X and Y (aw words), Z until the batch inversion
// (jw - aw words), the inversion's prefix products (one Fp) -- each an SoA over
// the chunk's rounds * t * 8 entries (a shorter last chunk uses a prefix of
// every region).  recw_chunk_rounds sizes `rounds` under RECW_TABLE_BUDGET.
struct rec_tab_wide_layout {
  uint32_t *tab, *tabz, *pre;
  void fill(carver& c, size_t rounds, size_t t, int aw, int jw) {
    const size_t ne = rounds * t * 8;
    tab = c.take<uint32_t>(ne * aw);
    tabz = c.take<uint32_t>(ne * (jw - aw));
    pre = c.take<uint32_t>(ne * FP_WORDS);
  }
};
// rec_part: the MSM's per-slice sums, slice i a Jacobian SoA of jw words per
// round with stride n_rounds (the kernels take the base: part + i * jw *
// n_rounds).  Sized for G2 points whatever the group.
struct rec_part_layout {
  static constexpr int SLICES = 5;
  uint32_t* slice[SLICES];
  uint32_t* spare;
  void fill(carver& c, size_t n_rounds, int jw) {
    for (uint32_t*& s : slice) s = c.take<uint32_t>(n_rounds * jw);
    spare = c.take<uint32_t>(n_rounds * SLICES * (G2J_WORDS - jw));
  }
};

}  // namespace dgpu
