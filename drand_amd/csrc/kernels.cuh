// Batch kernels: one thread per beacon round.  Intermediate points live in
// HBM as structure-of-arrays ([limb][round], round fastest) so every limb
// load/store of a wavefront is one coalesced 256-byte access.
#pragma once
#include <hip/hip_runtime.h>
#include "h2c.cuh"

namespace dgpu {

constexpr int FP_WORDS = FP_LIMBS;          // 14 dwords per Fp in HBM
constexpr int G2A_WORDS = 4 * FP_WORDS;     // affine G2 point

__device__ __forceinline__ void st_fp(uint32_t* base, size_t n, size_t i, const fp& a) {
#pragma unroll
  for (int k = 0; k < FP_LIMBS; ++k) base[(size_t)k * n + i] = a.l[k];
}
__device__ __forceinline__ fp ld_fp(const uint32_t* base, size_t n, size_t i) {
  fp a;
#pragma unroll
  for (int k = 0; k < FP_LIMBS; ++k) a.l[k] = base[(size_t)k * n + i];
  return a;
}
__device__ __forceinline__ void st_g2a(uint32_t* base, size_t n, size_t i, const g2a& p) {
  st_fp(base, n, i, p.x.c0);
  st_fp(base + FP_WORDS * n, n, i, p.x.c1);
  st_fp(base + 2 * FP_WORDS * n, n, i, p.y.c0);
  st_fp(base + 3 * FP_WORDS * n, n, i, p.y.c1);
}
__device__ __forceinline__ g2a ld_g2a(const uint32_t* base, size_t n, size_t i) {
  g2a p;
  p.x.c0 = ld_fp(base, n, i);
  p.x.c1 = ld_fp(base + FP_WORDS * n, n, i);
  p.y.c0 = ld_fp(base + 2 * FP_WORDS * n, n, i);
  p.y.c1 = ld_fp(base + 3 * FP_WORDS * n, n, i);
  return p;
}

constexpr int G2J_WORDS = 6 * FP_WORDS;

__device__ __forceinline__ void st_g2j(uint32_t* base, size_t n, size_t i, const g2j& p) {
  st_fp(base, n, i, p.x.c0);
  st_fp(base + FP_WORDS * n, n, i, p.x.c1);
  st_fp(base + 2 * FP_WORDS * n, n, i, p.y.c0);
  st_fp(base + 3 * FP_WORDS * n, n, i, p.y.c1);
  st_fp(base + 4 * FP_WORDS * n, n, i, p.z.c0);
  st_fp(base + 5 * FP_WORDS * n, n, i, p.z.c1);
}
__device__ __forceinline__ g2j ld_g2j(const uint32_t* base, size_t n, size_t i) {
  g2j p;
  p.x.c0 = ld_fp(base, n, i);
  p.x.c1 = ld_fp(base + FP_WORDS * n, n, i);
  p.y.c0 = ld_fp(base + 2 * FP_WORDS * n, n, i);
  p.y.c1 = ld_fp(base + 3 * FP_WORDS * n, n, i);
  p.z.c0 = ld_fp(base + 4 * FP_WORDS * n, n, i);
  p.z.c1 = ld_fp(base + 5 * FP_WORDS * n, n, i);
  return p;
}

// Test hook of the A/B build (DGPU_TEST_FORCE_EXC=1 at dgpu_open): the fast
// group-law paths (cofactor ladder, membership ladder, MSM additions) take
// their generic redo as if an exceptional addition had occurred, so the redo
// code runs on every item.  Always false in the shipped build.
#ifdef DG_AB_KNOBS
__device__ int g_dg_force_exc = 0;
#define DG_FORCE_EXC (g_dg_force_exc != 0)
#else
#define DG_FORCE_EXC false
#endif

// per-round status codes carried between kernels (also the public `reason`)
enum : uint8_t {
  ST_OK = 0,
  ST_DECODE = 1,    // wrong length / flags / x >= p / not on curve / non-canonical infinity
  ST_SUBGROUP = 2,  // point not in the r-order subgroup
  ST_PAIRING = 3,   // e(pk, H(m)) != e(g1, sig)
  ST_INFINITY = 4,  // signature is the point at infinity (pairing check fails)
};

struct g1_key {  // public key prepared for line evaluation: (-x, y), Montgomery
  fp neg_x, y;
};

// Where a batch item's message comes from: drand's DigestMessage of a beacon
// record (chain/verify.go:24-32: SHA-256(prev || BE64(round)), prev ignored
// unless chained), or raw message bytes (msgs != nullptr: key.Scheme.
// VerifyRecovered(pk, msg, sig) with any msg, key/curve.go:36-39,
// chain/beacon/chain.go:165).  A record whose length exceeds its stride
// (prev_len > prev_stride, msg_len > msg_stride) is never read past the
// stride and fails verification (msg_bad_record -> ST_DECODE).
struct msg_src {
  const uint64_t* rounds;
  const uint8_t* prev;
  size_t prev_stride;
  const uint32_t* prev_len;
  int chained;
  const uint8_t* msgs;
  size_t msg_stride;
  const uint32_t* msg_len;
};

// The linked form (dgpu_verify_segment) is a beacon record that is not
// stored: the walk of client/verify.go:118-178 builds each beacon from the
// signature before it, so item i of a slice whose first item is global item
// g0 has g = g0 + i, round first_round + g, and as previous signature the
// seed (carried by value: nothing of the caller's is read after the launch)
// when g == 0, else signature g - 1 of the call's own signature array --
// prev / prev_stride / prev_len are that array's *base*, whatever the slice,
// because a slice's first item reads the record before the slice.
//
// A type of its own, selected at compile time: every kernel that takes a
// message source is a template over it and reaches it only through
// msg_bad_record / msg_digest / msg_expand.  Behind a run-time flag of
// msg_src the seed's SHA-256 stream cost the explicit-record kernels 96 bytes
// of scratch (k_h2c_field) and spills in the two G1 hash kernels
// (profiles/r08/segment_resource_usage.txt); as instantiated for msg_src they
// are the kernels they were.  The host holds every source as one type
// (capi.hip msg_src_host) and `linked` tells which device type it is.
struct msg_src_linked : msg_src {
  int linked;         // host-side selector of the instantiation (SRC_*); the device type is always linked
  uint32_t seed_len;  // <= 96
  uint64_t first_round;
  size_t g0;
  uint32_t seed[24];  // 96 bytes, byte k in bits 8 (k % 4) of word k / 4
};

// One shard of a linked segment (dgpu_verify_segment_shard_device, the later
// shards of dgpu_verify_segment_multi): the linked form whose item 0 takes its
// previous signature from a one-record *halo* in device memory -- the
// neighbouring shard's last record, wherever a copy or a collective put it --
// read through pointers when the kernel runs, so it is ordered by the stream
// and nothing of it is known to the host at the launch.  The halo is a record
// like any other of the array: min(*halo_len, prev_stride) bytes at `halo`,
// and *halo_len > prev_stride makes item 0 a bad record, exactly as record
// g - 1's length does for item g.  first_round is the shard's own first
// round, prev / prev_len the shard's own signature arrays.  An unchained
// source never touches the halo pointers (they may be null).  No seed by
// value: the kernels instantiated for it carry the explicit form's arguments
// and no SHA-256 stream over kernel-argument words
// (profiles/r11/halo_resource_usage.txt).
struct msg_src_halo : msg_src {
  uint64_t first_round;
  size_t g0;
  const uint8_t* halo;
  const uint32_t* halo_len;
};

// msg_src_linked::linked on the host: which instantiation a source selects
enum : int { SRC_RECORDS = 0, SRC_LINKED = 1, SRC_HALO = 2 };

DG_FN uint32_t clamp_len(uint32_t len, size_t stride) {
  return (size_t)len > stride ? (uint32_t)stride : len;
}

// Round number of item i of a beacon source; whether its previous signature
// is the linked form's seed; the index of the record that holds its previous
// signature otherwise (i itself, or in the linked form the signature before
// it, global item g - 1); that record's bytes and its length as stored (not
// clamped) -- in the halo form the halo's for global item 0.
DG_FN uint64_t msg_round(const msg_src& m, size_t i) { return m.rounds[i]; }
DG_FN uint64_t msg_round(const msg_src_linked& m, size_t i) { return m.first_round + (m.g0 + i); }
DG_FN uint64_t msg_round(const msg_src_halo& m, size_t i) { return m.first_round + (m.g0 + i); }
DG_FN bool msg_prev_is_seed(const msg_src&, size_t) { return false; }
DG_FN bool msg_prev_is_seed(const msg_src_linked& m, size_t i) { return m.g0 + i == 0; }
DG_FN size_t msg_prev_index(const msg_src&, size_t i) { return i; }
DG_FN size_t msg_prev_index(const msg_src_linked& m, size_t i) { return m.g0 + i - 1; }
template <class Src>
DG_FN const uint8_t* msg_prev_ptr(const Src& m, size_t i) {
  return m.prev + msg_prev_index(m, i) * m.prev_stride;
}
template <class Src>
DG_FN uint32_t msg_prev_len(const Src& m, size_t i) {
  return m.prev_len[msg_prev_index(m, i)];
}
DG_FN const uint8_t* msg_prev_ptr(const msg_src_halo& m, size_t i) {
  const size_t g = m.g0 + i;
  return g == 0 ? m.halo : m.prev + (g - 1) * m.prev_stride;
}
DG_FN uint32_t msg_prev_len(const msg_src_halo& m, size_t i) {
  const size_t g = m.g0 + i;
  return *(g == 0 ? m.halo_len : m.prev_len + (g - 1));
}

// SHA-256(seed || BE64(round)): the digest of the linked form's first item.
// The seed word is picked by selects over constant indices, not by an indexed
// load (which would first copy the kernel argument to scratch).
DG_FN void msg_seed_digest(const msg_src&, uint64_t, uint32_t*) {}
DG_FN void msg_seed_digest(const msg_src_linked& m, uint64_t round, uint32_t msg[8]) {
  const uint32_t plen = m.seed_len;
  sha_state s = sha_init();
  sha_stream(s, plen + 8, 0, [&](uint32_t pos) -> uint32_t {
    if (pos >= plen) return (uint32_t)(round >> (8 * (7 - (pos - plen)))) & 0xffu;
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 24; ++k) w = (pos >> 2) == k ? m.seed[k] : w;
    return (w >> (8 * (pos & 3))) & 0xffu;
  });
  for (int w = 0; w < 8; ++w) msg[w] = s.h[w];
}

template <class Src>
DG_FN bool msg_bad_record(const Src& m, size_t i) {
  if (m.msgs) return (size_t)m.msg_len[i] > m.msg_stride;
  if (!m.chained || msg_prev_is_seed(m, i)) return false;
  return (size_t)msg_prev_len(m, i) > m.prev_stride;
}

// drand digest of a beacon record (32 bytes as 8 big-endian words)
template <class Src>
DG_FN void msg_digest(const Src& m, size_t i, uint32_t msg[8]) {
  const uint64_t round = msg_round(m, i);
  if (m.chained && msg_prev_is_seed(m, i)) {
    msg_seed_digest(m, round, msg);
    return;
  }
  const uint32_t plen = m.chained ? clamp_len(msg_prev_len(m, i), m.prev_stride) : 0u;
  drand_digest(msg, m.chained ? msg_prev_ptr(m, i) : nullptr, plen, round);
}

// expand_message_xmd of item i's message under DST G1DST with ELL 32-byte blocks
template <bool G1DST, int ELL, class Src>
DG_FN void msg_expand(const Src& m, size_t i, uint32_t* uni) {
  if (m.msgs) {
    expand_xmd_var<G1DST, ELL>(uni, m.msgs + i * m.msg_stride, clamp_len(m.msg_len[i], m.msg_stride));
  } else {
    uint32_t msg[8];
    msg_digest(m, i, msg);
    expand_xmd<G1DST, ELL>(uni, msg);
  }
}

// ---------------------------------------------------------------- k_h2c_finish's park region
// The three point slots of g2_clear_cofactor_stash as a register extension in
// HBM, blocked by wave: a block is 64 consecutive rounds, and slot k (0..2) of
// a block holds each round's 84 words (w = coord * 28 + comp * 14 + limb) as
// 21 quads, [block][slot][quad][lane][4].  One wave's point is 21 KB
// contiguous and an Fp2 coordinate (28 words = 7 quads) moves as seven
// 16-byte accesses per lane, 1 KB per wave each -- where the round's own SoA
// words ([coord][limb][n]) cost 84 dword accesses to planes 4n bytes apart on
// every fetch of the ladder's critical path.
constexpr int PARK_LANES = 64;
constexpr int PARK_SLOTS = 3;
constexpr int PARK_COORD_QUADS = 2 * FP_WORDS / 4;  // 7
constexpr int PARK_QUADS = 3 * PARK_COORD_QUADS;    // 21
static_assert(2 * FP_WORDS % 4 == 0, "an Fp2 coordinate is a whole number of quads");
// word offset of word w (0..83) of round i's slot k
DG_FN size_t h2c_park_word(size_t i, int k, int w) {
  return ((((i / PARK_LANES) * PARK_SLOTS + k) * PARK_QUADS + w / 4) * PARK_LANES + i % PARK_LANES) * 4 + w % 4;
}
// words of the region for n rounds: whole blocks, so the last partial block
// lies inside it for every n (sized per round it would not: DESIGN 2b')
DG_FN size_t h2c_park_words(size_t n) {
  return (n + PARK_LANES - 1) / PARK_LANES * PARK_LANES * (size_t)(PARK_SLOTS * G2J_WORDS);
}

struct h2c_finish_stash {
  uint32_t* park;  // 16-byte aligned, h2c_park_words(n) words
  size_t i;
  // word j (0..27) of an Fp2 coordinate: c0's limbs, then c1's
  static DG_FN uint32_t& word(fp2& a, int j) { return j < FP_WORDS ? a.c0.l[j] : a.c1.l[j - FP_WORDS]; }
  static DG_FN void st_coord(uint4* q, fp2 a) {
#pragma unroll
    for (int t = 0; t < PARK_COORD_QUADS; ++t)
      q[(size_t)t * PARK_LANES] = make_uint4(word(a, 4 * t), word(a, 4 * t + 1), word(a, 4 * t + 2), word(a, 4 * t + 3));
  }
  static DG_FN fp2 ld_coord(const uint4* q) {
    fp2 a;
#pragma unroll
    for (int t = 0; t < PARK_COORD_QUADS; ++t) {
      const uint4 v = q[(size_t)t * PARK_LANES];
      word(a, 4 * t) = v.x, word(a, 4 * t + 1) = v.y, word(a, 4 * t + 2) = v.z, word(a, 4 * t + 3) = v.w;
    }
    return a;
  }
  struct fetch {  // slot k's coordinates, each loaded where g2_add_nx_q uses it
    const uint4* q;  // the round's quad 0 of the slot
    DG_FN fp2 x() const { return ld_coord(q); }
    DG_FN fp2 y() const { return ld_coord(q + (size_t)PARK_COORD_QUADS * PARK_LANES); }
    DG_FN fp2 z() const { return ld_coord(q + (size_t)2 * PARK_COORD_QUADS * PARK_LANES); }
  };
  DG_FN uint4* slot(uint32_t* base, int k) const { return (uint4*)(base + h2c_park_word(i, k, 0)); }
  DG_FN void put(int k, const g2j& p) {
    uint4* q = slot(park, k);
    st_coord(q, p.x);
    st_coord(q + (size_t)PARK_COORD_QUADS * PARK_LANES, p.y);
    st_coord(q + (size_t)2 * PARK_COORD_QUADS * PARK_LANES, p.z);
  }
  // (the base passes through an empty asm: the slot is re-read at each
  // addition instead of hoisted out of the ladder and spilled)
  DG_FN fetch at(int k) const {
    uint32_t* b = park;
#ifdef __HIP_DEVICE_COMPILE__
    __asm__ volatile("" : "+s"(b));
#endif
    return fetch{slot(b, k)};
  }
  DG_FN g2j get(int k) const {
    const fetch f{slot(park, k)};
    return g2j{f.x(), f.y(), f.z()};
  }
};

#ifndef DG_NO_KERNELS  // (a host-only test program takes the helpers above alone)
// ---------------------------------------------------------------- kernels
// The per-round hash to G2 as three launches (the fused kernel needs 512
// registers per lane -- one wave per SIMD -- and 6 KB of scratch; each stage
// alone is far lighter, and the SSWU stage has 2n independent items):
//   k_h2c_field   message (DigestMessage or raw) + expand_message_xmd -> u0, u1 ([4 fp][n])
//   k_h2c_sswu    SSWU + 3-isogeny of each of the 2n field elements -> Jacobian ([2][6 fp][n])
//   k_h2c_finish  Q0 + Q1, cofactor clearing -> X, Y (h_out) and Z (z_out)
template <class Src>
__global__ void __launch_bounds__(256) k_h2c_field(size_t n, Src m, uint32_t* __restrict__ u_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t uni[64];
  msg_expand<false, 8>(m, i, uni);
#pragma unroll 1
  for (int k = 0; k < 4; ++k) st_fp(u_out + (size_t)k * FP_WORDS * n, n, i, fp_from_be64_words(uni + 16 * k));
}

// Minimum blocks per CU of the two heavy hash kernels (A/B knobs).
#ifndef DG_SSWU_OCC
#define DG_SSWU_OCC 2
#endif
#ifndef DG_FINISH_OCC
#define DG_FINISH_OCC 2
#endif
__global__ void __launch_bounds__(256, DG_SSWU_OCC) k_h2c_sswu(size_t n, const uint32_t* __restrict__ u,
                                                   uint32_t* __restrict__ q_out) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * n) return;
  const size_t which = j / n, i = j % n;
  const uint32_t* ub = u + which * 2 * FP_WORDS * n;
  const fp2 uu{ld_fp(ub, n, i), ld_fp(ub + FP_WORDS * n, n, i)};
  st_g2j(q_out + which * G2J_WORDS * n, n, i, map_to_curve_sswu_iso3_body(uu));
}

// (The SSWU stage in five launches, the two exponentiations of each item alone
// in a 90-VGPR kernel at 5 waves per SIMD, was measured slower in the bulk
// pass: profiles/r06/r06i_sswu_staged_occupancy_ab.txt; the code is in git
// history.)

// An affine point at item i of an SoA array ([x.c0, x.c1, y.c0, y.c1][limb][n]),
// each coordinate loaded where the ladder uses it (the base passes through an
// empty asm per fetch so the loads stay in the loop instead of being hoisted
// and spilled).
struct g2a_soa_fetch {
  const uint32_t* base;
  size_t n, i;
  __device__ __forceinline__ const uint32_t* b() const {
    const uint32_t* p = base;
    __asm__ volatile("" : "+s"(p));
    return p;
  }
  __device__ __forceinline__ fp2 x() const {
    const uint32_t* p = b();
    return fp2{ld_fp(p, n, i), ld_fp(p + FP_WORDS * n, n, i)};
  }
  __device__ __forceinline__ fp2 y() const {
    const uint32_t* p = b();
    return fp2{ld_fp(p + 2 * FP_WORDS * n, n, i), ld_fp(p + 3 * FP_WORDS * n, n, i)};
  }
  __device__ __forceinline__ g2a get() const { return g2a{x(), y()}; }
};
// G2 membership of a decoded signature p, stored first at item i of pts (its
// output slot): the ladder form, the generic test on an exceptional addition.
__device__ __forceinline__ bool g2_in_subgroup_stored(const g2a& p, uint32_t* pts, size_t n, size_t i) {
  st_g2a(pts, n, i, p);
  bool exc = false;
  const g2a_soa_fetch f{pts, n, i};
  const bool in = g2_in_subgroup_ladder(p, f, exc);
  return exc || DG_FORCE_EXC ? g2_in_subgroup(g2_from_affine(f.get())) : in;
}

// Q0 + Q1 and the cofactor clearing, its cold points parked in HBM (one
// point live per [|x|] ladder, no call sites in the loops; VERDICT r05 item
// 3) in the wave-blocked slots of `park` (h2c_finish_stash).  An exceptional
// addition on the fast path (Q0 = +-Q1, a small-order point, ...) flags the
// round in `redo`, and k_h2c_finish_redo recomputes it from P, which slot 0
// still holds.  The redo is a kernel of its own because a kernel is allotted
// the registers of everything it can call: g2_clear_cofactor and
// g2_clear_cofactor_generic take 256 and 32 accumulation registers, and with
// the call in this kernel it ran at one wave per SIMD instead of two
// (profiles/r09/finish_pmc_change.txt: 65.2 against 45.9 ms per 1M rounds).
__device__ __forceinline__ void st_h2c_out(uint32_t* h_out, uint32_t* z_out, size_t n, size_t i, const g2j& h) {
  st_g2a(h_out, n, i, g2a{h.x, h.y});
  st_fp(z_out, n, i, h.z.c0);
  st_fp(z_out + FP_WORDS * n, n, i, h.z.c1);
}
__global__ void __launch_bounds__(256, DG_FINISH_OCC) k_h2c_finish(size_t n, const uint32_t* __restrict__ q,
                                                     uint32_t* __restrict__ park, uint8_t* __restrict__ redo,
                                                     uint32_t* __restrict__ h_out, uint32_t* __restrict__ z_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  h2c_finish_stash st{park, i};
  bool exc = false;
  const g2j h = g2_clear_cofactor_stash(ld_g2j(q, n, i), ld_g2j(q + G2J_WORDS * n, n, i), st, exc);
  redo[i] = exc || DG_FORCE_EXC;
  st_h2c_out(h_out, z_out, n, i, h);
}
__global__ void __launch_bounds__(256) k_h2c_finish_redo(size_t n, const uint8_t* __restrict__ redo, uint32_t* park,
                                                         uint32_t* __restrict__ h_out, uint32_t* __restrict__ z_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !redo[i]) return;
  const h2c_finish_stash st{park, i};
  st_h2c_out(h_out, z_out, n, i, DG_FORCE_EXC ? g2_clear_cofactor_generic(st.get(0)) : g2_clear_cofactor(st.get(0)));
}

// RLC mode's pre-cofactor hash point R = Q0 + Q1 (Jacobian, [6 fp][n]) from
// k_h2c_sswu's output: the cofactor is cleared once per checked tree node.
__global__ void __launch_bounds__(256, 2) k_h2c_sum(size_t n, const uint32_t* __restrict__ q,
                                                  uint32_t* __restrict__ r_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_g2j(r_out, n, i, g2_add_body(ld_g2j(q, n, i), ld_g2j(q + G2J_WORDS * n, n, i)));
}

// Jacobian -> affine for n G2 points in place (X, Y in pts; Z in z) with one
// Fp inversion per thread: thread t takes points t, t + T, ... (T threads in
// the grid) and inverts the norms N(Z_i) by Montgomery's trick (prefix
// products in `pre`); 1/Z = conj(Z) / N(Z).  Z = 0 (the identity) gives (0, 0)
// like g2_to_affine.
__global__ void __launch_bounds__(256) k_g2_batch_affine(size_t n, uint32_t* __restrict__ pts,
                                                         const uint32_t* __restrict__ z, uint32_t* __restrict__ pre) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  auto ldz = [&](size_t i) { return fp2{ld_fp(z, n, i), ld_fp(z + FP_WORDS * n, n, i)}; };
  fp acc = fp_one();
  size_t last = t;
  for (size_t i = t; i < n; i += T) {
    const fp nz = fp2_norm(ldz(i));
    acc = fp_mul(acc, fp_cmov(nz, fp_one(), fp_is_zero(nz)));
    st_fp(pre, n, i, acc);
    last = i;
  }
  fp inv = fp_inv(acc);
  for (size_t i = last;; i -= T) {
    const fp2 zi = ldz(i);
    const fp nz = fp2_norm(zi);
    const bool inf = fp_is_zero(nz);
    const fp ninv = i >= t + T ? fp_mul(inv, ld_fp(pre, n, i - T)) : inv;  // 1 / N(Z_i)
    const fp2 zinv = fp2_mul_fp(fp2_conj(zi), ninv);
    const fp2 zinv2 = fp2_sqr(zinv);
    g2a a = ld_g2a(pts, n, i);
    a.x = fp2_mul(a.x, zinv2);
    a.y = fp2_mul(a.y, fp2_mul(zinv2, zinv));
    st_g2a(pts, n, i, inf ? g2a{fp2_zero(), fp2_zero()} : a);
    if (i < t + T) break;
    if (!inf) inv = fp_mul(inv, nz);
  }
}

// H(m) for raw messages of any length, compressed (parity surface:
// dgpu_hash_to_g2 / dgpu_hash_to_curve)
__global__ void __launch_bounds__(256) k_hash_to_g2_msgs(size_t n, msg_src m, uint8_t* __restrict__ out96) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t uni[64];
  msg_expand<false, 8>(m, i, uni);
  const fp2 u0{fp_from_be64_words(uni), fp_from_be64_words(uni + 16)};
  const fp2 u1{fp_from_be64_words(uni + 32), fp_from_be64_words(uni + 48)};
  g2j h = g2_clear_cofactor(g2_add(map_to_curve_sswu_iso3(u0), map_to_curve_sswu_iso3(u1)));
  bool inf = g2_is_inf(h);
  g2a a = inf ? g2a{fp2_zero(), fp2_zero()} : g2_to_affine(h);
  g2_compress(out96 + i * 96, a, inf);
}

// drand digests only (parity/debug: dgpu_digest)
__global__ void __launch_bounds__(256) k_digest(size_t n, const uint64_t* __restrict__ rounds,
                                                 const uint8_t* __restrict__ prev, size_t prev_stride,
                                                 const uint32_t* __restrict__ prev_len, int chained,
                                                 uint8_t* __restrict__ out32) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[8];
  drand_digest(msg, chained ? prev + i * prev_stride : nullptr, chained ? prev_len[i] : 0u, rounds[i]);
  for (int w = 0; w < 8; ++w) {
    out32[i * 32 + 4 * w] = (uint8_t)(msg[w] >> 24);
    out32[i * 32 + 4 * w + 1] = (uint8_t)(msg[w] >> 16);
    out32[i * 32 + 4 * w + 2] = (uint8_t)(msg[w] >> 8);
    out32[i * 32 + 4 * w + 3] = (uint8_t)msg[w];
  }
}

// Signature decode (kilic G2.FromCompressed semantics (R)) + G2 membership.
// A record whose message part overruns its stride (msg_bad_record) fails as a
// decode error without its signature being read.  check_subgroup = 0: the
// membership test is left to the pairing engine's lines kernel (the Miller
// loop's ladder of the signature gives [x] sig for free, k_eng_lines).
template <class Src>
__global__ void __launch_bounds__(256, 4) k_decode_g2_sigs(size_t n, const uint8_t* __restrict__ sigs, size_t sig_stride,
                                                         const uint32_t* __restrict__ sig_len, Src m,
                                                         int check_subgroup, uint32_t* __restrict__ sig_out,
                                                         uint8_t* __restrict__ status) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t st;
  g2a p{fp2_zero(), fp2_zero()};
  if (sig_len[i] != 96 || msg_bad_record(m, i)) {
    st = ST_DECODE;
  } else {
    uint8_t buf[96];
    const uint8_t* src = sigs + i * sig_stride;
    for (int k = 0; k < 96; ++k) buf[k] = src[k];
    int rc = g2_decompress(&p, buf, check_subgroup != 0);
    st = rc == DEC_OK ? ST_OK : rc == DEC_INFINITY ? ST_INFINITY : rc == DEC_ERR_SUBGROUP ? ST_SUBGROUP : ST_DECODE;
  }
  st_g2a(sig_out, n, i, p);
  status[i] = st;
}

// The same decode with the G2 membership check (RLC mode and recovery need
// it up front; DGPU_SUBGROUP=decode): the 63-doubling ladder inlined into
// the kernel at 2 waves/SIMD -- out of line in g2_decompress its registers
// escaped the kernel's budget (4.6 KB of scratch at 4 waves/SIMD): 389.6 ->
// 360.2 ms per 10M (tools/engbench/dec_g2.hip, profiles/r04/r04f_dec_g2_variants.txt).
template <class Src>
__global__ void __launch_bounds__(256, 2) k_decode_g2_sigs_sub(size_t n, const uint8_t* __restrict__ sigs,
                                                             size_t sig_stride, const uint32_t* __restrict__ sig_len,
                                                             Src m, uint32_t* __restrict__ sig_out,
                                                             uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t st;
  g2a p{fp2_zero(), fp2_zero()};
  if (sig_len[i] != 96 || msg_bad_record(m, i)) {
    st = ST_DECODE;
    st_g2a(sig_out, n, i, p);
  } else {
    uint8_t buf[96];
    const uint8_t* src = sigs + i * sig_stride;
    for (int k = 0; k < 96; ++k) buf[k] = src[k];
    int rc = g2_decompress(&p, buf, false);
    if (rc == DEC_OK) {  // p is stored by the membership test (not kept live across its ladder)
      if (!g2_in_subgroup_stored(p, sig_out, n, i)) rc = DEC_ERR_SUBGROUP;
    } else {
      st_g2a(sig_out, n, i, p);
    }
    st = rc == DEC_OK ? ST_OK : rc == DEC_INFINITY ? ST_INFINITY : rc == DEC_ERR_SUBGROUP ? ST_SUBGROUP : ST_DECODE;
  }
  status[i] = st;
}

// Synthetic-chain generator (test-data tool, not the verify path): one step
// of S independent chained segments, following the reference's fixture
// generator client/test/result/mock/result.go:86-130 (msg = DigestMessage,
// sig = sk * H(msg), previous = sig).  Segment s signs round first_round[s] + step
// over prev (prev_len[s] bytes at prev + s*96) and writes the 96-byte
// signature to sig_out + s*96 and to prev (for the next step).
struct scalar256 {
  uint32_t w[8];
};
__global__ void __launch_bounds__(256) k_sign_step(size_t S, const uint64_t* __restrict__ first_round, uint64_t step,
                                                    uint8_t* __restrict__ prev, uint32_t* __restrict__ prev_len,
                                                    int chained, scalar256 sk, uint8_t* __restrict__ sig_out,
                                                    size_t sig_stride) {
  size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  uint32_t msg[8];
  uint8_t pb[96];
  uint32_t plen = chained ? prev_len[s] : 0u;
  for (uint32_t k = 0; k < plen && k < 96; ++k) pb[k] = prev[s * 96 + k];
  drand_digest(msg, pb, plen, first_round[s] + step);
  g2j h = hash_to_g2(msg);
  g2j sg = g2_mul_words(h, sk.w, 8);
  bool inf = g2_is_inf(sg);
  g2a a = inf ? g2a{fp2_zero(), fp2_zero()} : g2_to_affine(sg);
  uint8_t out[96];
  g2_compress(out, a, inf);
  for (int k = 0; k < 96; ++k) {
    sig_out[s * sig_stride + k] = out[k];
    prev[s * 96 + k] = out[k];
  }
  prev_len[s] = 96;
}

// pk = sk * g1, compressed (synthetic-chain tool)
__global__ void k_derive_pubkey(scalar256 sk, uint8_t* __restrict__ out48) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  g1j g{C_G1_X, C_G1_Y, fp_one()};
  g1j p = g1_mul_words(g, sk.w, 8);
  bool inf = g1_is_inf(p);
  g1a a = inf ? g1a{fp_zero(), fp_zero()} : g1_to_affine(p);
  uint8_t out[48];
  g1_compress(out, a, inf);
  for (int k = 0; k < 48; ++k) out48[k] = out[k];
}

// ================================================================ RLC batching
// Shared-key collapse of the random linear combination:
//   prod_i d_i^{r_i} = e(pk, h_eff * sum_i r_i R_i) * e(-g1, sum_i r_i sig_i),
// with R_i the pre-cofactor hash point (h_eff applied once per checked node,
// by linearity) and d_i = e(pk, H_i) e(-g1, sig_i).  Jacobian G2 arrays are
// SoA [6 Fp][limb][index].
// SplitMix64-derived nonzero 64-bit coefficient for batch position `idx`
// under `seed`.  Keyed on the position, never on the record's Round field:
// two records with equal Round (duplicated store rows) must get independent
// coefficients, or a +D / -D pair of corruptions cancels in every node.
__device__ __forceinline__ uint64_t rlc_coeff(uint64_t seed, uint64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z ? z : 1ull;
}

// Node status of a trivially passing candidate (both points at infinity;
// rlc_msm.cuh k_rlc_prep).
constexpr uint8_t RLC_TRIVIAL = 0x80;

// Engine verdicts of the candidates -> fail flags.
__global__ void __launch_bounds__(256) k_rlc_fail(size_t n_cand, const uint8_t* __restrict__ st,
                                                  uint8_t* __restrict__ fail) {
  size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  fail[c] = (st[c] == ST_OK || st[c] == RLC_TRIVIAL) ? 0 : 1;
}

// Mark the rounds of failing leaves.
__global__ void k_rlc_mark(size_t n_cand, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ fail,
                           uint8_t* __restrict__ status) {
  size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  if (fail[c]) status[idx[c]] = ST_PAIRING;
}

// status -> verdict bitmap (bit = 1 valid), one thread per output byte
__global__ void k_pack_verdicts(size_t n, const uint8_t* __restrict__ status, uint8_t* __restrict__ bits) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j * 8 >= n) return;
  uint8_t b = 0;
  for (int k = 0; k < 8; ++k) {
    size_t i = j * 8 + k;
    if (i < n && status[i] == ST_OK) b |= (uint8_t)(1u << k);
  }
  bits[j] = b;
}

// Randomness of the verified rounds (dgpu_verify_segment, after the status is
// final): out32 + 32 i = SHA-256 of round i's signature where status[i] ==
// ST_OK (its length is then exactly the scheme's 48 or 96 bytes, within the
// stride), 32 zero bytes otherwise.
__global__ void __launch_bounds__(256) k_randomness(size_t n, const uint8_t* __restrict__ sigs, size_t sig_stride,
                                                     const uint32_t* __restrict__ sig_len,
                                                     const uint8_t* __restrict__ status, uint8_t* __restrict__ out32) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t* o = out32 + i * 32;
  if (status[i] == ST_OK) {
    sha256_bytes(o, sigs + i * sig_stride, clamp_len(sig_len[i], sig_stride));
  } else {
    for (int k = 0; k < 32; ++k) o[k] = 0;
  }
}

// nonzero bytes -> bitmap (bit = 1 where ok[i] != 0): recovery verdicts
__global__ void k_pack_ok(size_t n, const uint8_t* __restrict__ ok, uint8_t* __restrict__ bits) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j * 8 >= n) return;
  uint8_t b = 0;
  for (int k = 0; k < 8; ++k) {
    size_t i = j * 8 + k;
    if (i < n && ok[i]) b |= (uint8_t)(1u << k);
  }
  bits[j] = b;
}

// Public key decode (48-byte compressed G1, kilic G1.FromCompressed (R)) on one thread.
__global__ void k_decode_g1_pk(const uint8_t* __restrict__ in48, uint32_t* __restrict__ out, int* __restrict__ rc) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint8_t buf[48];
  for (int k = 0; k < 48; ++k) buf[k] = in48[k];
  g1a p{fp_zero(), fp_zero()};
  int r = g1_decompress(&p, buf, GROUP_ORDER_WORDS);
  fp nx = fp_neg(p.x);
  for (int k = 0; k < FP_LIMBS; ++k) {
    out[k] = nx.l[k];
    out[FP_LIMBS + k] = p.y.l[k];
  }
  *rc = r;
}

// Decoded points (SoA, nfp Fp coordinates of stride n, Montgomery) -> canonical
// big-endian 48-byte coordinates, item-major: out + (i nfp + j) 48.  neg_first:
// coordinate 0 is stored negated (k_decode_g1_pk's (-x, y)).  The decode
// entry points' readout (dgpu_decode_signatures / dgpu_decode_pubkey).
__global__ void __launch_bounds__(256) k_fp_soa_to_be48(size_t n, int nfp, const uint32_t* __restrict__ pts,
                                                        int neg_first, uint8_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (size_t)nfp) return;
  const size_t i = t / (size_t)nfp;
  const int j = (int)(t - i * (size_t)nfp);
  fp v = ld_fp(pts + (size_t)j * FP_WORDS * n, n, i);
  if (neg_first && j == 0) v = fp_neg(v);
  fp_std_to_be48(fp_from_mont(v), out + t * 48);
}

#endif  // DG_NO_KERNELS

}  // namespace dgpu
