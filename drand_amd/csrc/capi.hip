// libdrand_gpu.so: the C-ABI boundary (include/drand_gpu.h) over the gfx950
// kernels.  Host side of the product path: device memory, streams, launches,
// the per-context key cache and the multi-GPU (RCCL) driver.
// There is deliberately no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/drand_gpu.h"
#include "copy_pool.h"
#include "kernels.cuh"
#include "pairing_engine.cuh"
#include "miller6_kernels.cuh"
#include "feseg6_kernels.cuh"
#include "lines_thread.cuh"
#include "kb_thread.cuh"
#include "recover.cuh"
#include "g1sig.cuh"
#include "rlc_msm.cuh"
#include "recover_g1.cuh"
#include "recover_wide.cuh"
#include "ingest_row.cuh"
#include "check_rows.cuh"
#include "keyed.cuh"
#include "scratch_layouts.h"
#include "record_arrays.h"

using namespace dgpu;

namespace {

thread_local std::string g_last_error;

int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int set_err(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return set_err(DGPU_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)
// the same for the library's own int codes (the message is already set)
#define RC_TRY(expr)                  \
  do {                                \
    if (int _rc = (expr)) return _rc; \
  } while (0)

// Grow-only device scratch buffer, owner of its allocation.  Growth frees the
// old allocation only after the device is idle: a kernel enqueued earlier
// (this call or an earlier asynchronous one) may still read it.  The
// destructor and release() free at once: the owner has drained the streams
// that used the buffer (dgpu_close, stream_scratch, the callers of release()).
// as<T>() (u32() / u8() / u64() for the three common element types): the
// buffer as the element type a kernel takes; p itself is for the calls that
// want an untyped pointer (copies, memsets, layout_at, record_ptr_set).
#ifdef DG_AB_KNOBS
// test hook of the A/B build (DGPU_TEST_ALLOC_CAP=<bytes>): larger requests
// fail as an out-of-memory hipMalloc would (the engine chunk's retry path)
size_t g_test_alloc_cap = 0;
#endif
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return DGPU_OK;
#ifdef DG_AB_KNOBS
    if (g_test_alloc_cap && bytes > g_test_alloc_cap)
      return set_err(DGPU_ENOMEM, "hipMalloc(%zu): test cap %zu", bytes, g_test_alloc_cap);
#endif
    if (p) {
      (void)hipDeviceSynchronize();
      (void)hipFree(p);
    }
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) return set_err(DGPU_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    cap = bytes;
    return DGPU_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  uint32_t* u32() const { return as<uint32_t>(); }
  uint8_t* u8() const { return as<uint8_t>(); }
  uint64_t* u64() const { return as<uint64_t>(); }
};

// Size, allocate and carve a buffer with more than one region: the layout's
// one fill() (scratch_layouts.h) gives the bytes and then the pointers.
template <class L, class... D>
int carve(DevBuf& b, L* lay, D... dims) {
  int rc = b.ensure(layout_bytes<L>(dims...));
  if (rc) return rc;
  *lay = layout_at<L>(b.p, dims...);
  return DGPU_OK;
}

inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

// One checked kernel launch.  The argument types are the kernel's own
// parameter types (same<> keeps them out of deduction), so arity is checked
// and T* -> const T* and nullptr convert as in a direct call.  Nothing else
// happens here: no skip of an empty grid, no synchronisation, no stage mark.
template <class T>
struct same_t {
  using type = T;
};
template <class T>
using same = typename same_t<T>::type;
template <class... KA>
int launch(void (*k)(KA...), dim3 grid, dim3 block, hipStream_t s, same<KA>... a) {
  hipLaunchKernelGGL(k, grid, block, 0, s, a...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DGPU_OK : set_err(DGPU_EDEVICE, "kernel launch: %s", hipGetErrorString(e));
}
// ... of `threads` threads in one-dimensional blocks of `block`
template <class... KA>
int launch_n(void (*k)(KA...), size_t threads, unsigned block, hipStream_t s, same<KA>... a) {
  return launch(k, dim3(grid_for(threads, block)), dim3(block), s, a...);
}

// Fork or join of two streams: `waiter` continues after what `from` holds now.
inline int stream_after(hipStream_t waiter, hipStream_t from, hipEvent_t ev) {
  HIP_TRY(hipEventRecord(ev, from));
  HIP_TRY(hipStreamWaitEvent(waiter, ev, 0));
  return DGPU_OK;
}

// SplitMix64 step on the host: independent RLC seeds derived from a call's
// seed per device of dgpu_verify_multi (drand_amd/dist.py rank_seed is the
// same derivation per rank).  The confirmation check reuses the shard's seed:
// it subtracts terms from that seed's root.
uint64_t splitmix_host(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// signatures on G1 / public key on G2 (bls-unchained-on-g1, bls-unchained-g1-rfc9380)
inline bool sig_on_g1(int scheme) { return scheme == DGPU_SCHEME_UNCHAINED_G1 || scheme == DGPU_SCHEME_G1_RFC9380; }
inline bool scheme_known(int scheme) { return scheme >= DGPU_SCHEME_CHAINED && scheme <= DGPU_SCHEME_G1_RFC9380; }

// rounds per pairing-engine chunk (upper bound; dgpu_open lowers it to fit a
// quarter of the free HBM): the line buffer takes 45.7 KB per round (24 GB at
// 512Ki, per lane).  r01u A/B at 1M rounds: 64Ki 1.333M, 128Ki 1.362M,
// 256Ki 1.383M, 512Ki 1.394M rounds/s.
// Rounds per engine chunk and lane: 1Mi measured +0.4% over 512Ki on the
// 10M headline (per-thread lines and chains 4-5% faster per round, r04c1);
// at most half the free HBM (two lanes x ~53 KB per round = 112 GB at 1Mi).
constexpr size_t ENG_CHUNK = 1048576;
constexpr size_t ENG_CHUNK_MIN = 16384;
// per-round G2 batches of at least this many rounds run on two lanes
constexpr size_t LANE_MIN = 262144;
// decoded public keys cached per context (chain/verify.go:38 passes the key per call)
constexpr int KEY_SLOTS = 8;
// host-record staging (verify_status_host_locked): pinned ring slot size and
// the host threads that fill the slots
constexpr size_t STAGE_SLOT_BYTES = 16u << 20;
constexpr int STAGE_COPY_THREADS = 8;

// Per-round G2 path scratch of one "lane" (a stream working on a contiguous
// slice of the batch).  Two lanes overlap one slice's register-bound hash /
// decode kernels with the other slice's LDS-bound pairing engine.  Lane 0 is
// also the context's general scratch (RLC, recovery, the G1 path).
struct lane_scratch {
  DevBuf h_pts, sig_pts, h_z, h_pre, h_tmp;
  // pairing engine (per-round mode): per-chunk lines / f / norms / Karabina state
  DevBuf lines, f, n1, kb;
};

// One decoded public key: the engine's block constants carry its pairing
// point; G2 keys (G1-signature schemes) also own the fixed-Q line table.
struct key_entry {
  bool used = false;
  bool g2key = false;
  uint8_t bytes[96] = {};
  g1_key pk{};
  DevBuf consts, table;
  uint64_t stamp = 0;
};

// f(source) with the source as the type its kernels are instantiated for:
// the halo form, the linked form, or the msg_src part of any other.
template <class F>
auto with_src(const msg_src_host& m, F&& f) {
  if (m.linked == SRC_HALO) {
    msg_src_halo h{};
    static_cast<msg_src&>(h) = m;
    h.first_round = m.first_round;
    h.g0 = m.g0;
    h.halo = m.halo;
    h.halo_len = m.halo_len;
    return f(static_cast<const msg_src_halo&>(h));
  }
  return m.linked ? f(static_cast<const msg_src_linked&>(m)) : f(static_cast<const msg_src&>(m));
}
// the kernel template K for the source type of `src` (inside with_src)
#define SRC_KERNEL(K, src) K<std::decay_t<decltype(src)>>

// f(group) with the signature group as the type its kernels and host
// templates are instantiated for: G1Ops{} (signatures on G1) or G2Ops{}.
template <class F>
auto with_group(bool g1, F&& f) {
  return g1 ? f(G1Ops{}) : f(G2Ops{});
}
// the group type of `gr` (inside with_group)
#define GROUP_OF(gr) std::decay_t<decltype(gr)>

}  // namespace

struct dgpu_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // second lane of the per-round G2 path
  hipEvent_t lane_ev[2] = {nullptr, nullptr};
  hipEvent_t cof_ev[2] = {nullptr, nullptr};  // the small-call cofactor path's second-stream join
  // end of the last call's enqueued work: every call orders its stream after it
  hipEvent_t done = nullptr;
  std::mutex mu;
  key_entry keys[KEY_SLOTS];
  key_entry* cur = nullptr;  // key installed by dgpu_set_pubkey (dgpu_verify_batch[_device])
  uint64_t clock = 0;
  // engine block constants without a key (recovery: per-item keys)
  DevBuf eng_consts;
  // scratch
  lane_scratch lane[2];
  DevBuf status;
  // RLC mode: pre-cofactor hash points, segment-tree levels, bisection scratch
  DevBuf rlc_tree, rlc_idx, rlc_fail, rlc_h, rlc_s, rlc_st, rlc_root;
  // localize-then-confirm: the confirmation root + compacted list, the marked rounds' leaf sums
  DevBuf rlc_conf, rlc_fsum;
  // RLC root by bucket MSM (rlc_msm.cuh): AoS points, flags, counts / offsets /
  // cursors, bucket lists, bucket sums, per-run window sums
  DevBuf msm_aos, msm_flags, msm_counts, msm_list, msm_buckets, msm_runs, msm_root, msm_part;
  bool fe_gs = false;            // DGPU_FE=gs: the Granger-Scott FE kernel instead of the Karabina chain (A/B)
  size_t fe_gs_max = 16384;      // DGPU_FE_GS_MAX=<items>: pairing calls up to this size take the Granger-Scott FE
                                 // (one launch, no batched inversions: the latency path; 0 = always Karabina)
  size_t kb_inv_chain = 16;      // DGPU_KB_INV_CHAIN: norms per k_eng_inv thread in the Karabina FE (A/B)
  size_t kb_test_flag = 0;       // DGPU_KB_TEST_FLAG=k (tests): flag every k-th item so the fallback runs
  int lanes = 2;                 // DGPU_LANES=1: one stream (A/B)
  size_t lane_slices = 2;        // DGPU_LANE_SLICES: slices of a two-lane batch, alternating between the lanes
  size_t eng_chunk = ENG_CHUNK;  // DGPU_ENG_CHUNK=<rounds> or sized from free HBM
  size_t chunk_retries = 0;      // engine-chunk halvings after an out-of-memory allocation (eng_pairing_locked)
  bool kb_thread = true;         // DGPU_KB_CHAIN=lanes: the 8-lane compressed chain (k_eng_kb_chain, A/B)
  bool kb_norm_chain = true;     // the per-thread chain writes the six norms (r05c/r05d: kbinv -17%, FE -1.5%
                                 // same-box); DGPU_KB_NORM=planes: k_eng_kb_norm reads f1 from the planes (A/B;
                                 // the row-staged, image and round-fastest decompression variants measured in
                                 // r05c-r05j, all slower, are in git history)
  bool rlc_localize = true;      // DGPU_RLC_LOCALIZE=0: a failing RLC root goes straight to the random-coefficient tree (A/B)
  int rlc_descent_step = 3;      // DGPU_RLC_DESCENT_STEP: tree levels per descent step (children checked: 2^step; r04g: 3 > 2 > 5)
  bool lines_thread = true;      // DGPU_LINES=engine: T-steps on the 12-lane engine (k_eng_lines, A/B)
  bool miller6 = true;           // DGPU_MILLER=lanes12: the Miller product on the 12-lane engine (k_eng_miller) at every
                                 // size; default: chunks of thr_min items and more take k_eng_miller6 and the norm tail
  bool feseg6 = true;            // DGPU_FESEG=lanes12: the Karabina FE's segments 1..5 on the 12-lane engine (k_eng_fe_seg) at
                                 // every size; default: chunks of thr_min items and more take k_eng_fe_seg6
  size_t thr_min = 65536;        // DGPU_THR_MIN=<items>: pairing chunks smaller than this take the lane kernels,
                                 // which fill the chip and cut the per-item latency (RLC node checks, r04k: 11.15M
                                 // -> 11.49M rounds/s at 0.1% corrupted; small per-round batches, r04z)
  size_t rlc_min = 131072;       // DGPU_RLC_MIN=<rounds>: smaller RLC-mode batches run the per-round path (identical
                                 // verdicts; the root MSM's and the descent's fixed costs lose below ~150k rounds, r04x)
  bool fused_fixed = true;       // DGPU_G1_LINES=buffer: on-G1 lines through k_eng_lines_fixed (A/B)
  bool decode_subgroup = false;  // DGPU_SUBGROUP=decode: G2 membership in the decoder, not the lines kernel (A/B)
  // threshold group (dgpu_set_group): commitments, PubPoly.Eval table; recovery scratch
  int grp_t = 0, grp_n = 0;
  // the installed group's scheme (dgpu_set_group_scheme); a G1-signature
  // group (G2 commitments) owns C_0 as a decoded G2 key with its fixed-Q line
  // table, outside the caller's key cache, and the 96-byte round slots its
  // recovered signatures are packed from
  int grp_scheme = DGPU_SCHEME_CHAINED;
  bool grp_g1 = false;
  key_entry grp_key;
  DevBuf grp_stage, rec_slots;
  DevBuf grp_commits, grp_table, rec_msgs, rec_parts, rec_plen, rec_hidx, rec_pk, rec_idx, rec_lam, rec_out, rec_ok,
      rec_pts, rec_vpk, rec_sel, rec_part, rec_st;
  // batched recovery check: the group's window table of the share keys, round
  // classes, and the compact batch of rounds that take the exact path
  DevBuf grp_wtab, rec_cls, rec_x_list, rec_x_msgs, rec_x_parts, rec_x_plen, rec_x_out, rec_x_ok, rec_x_st;
  DevBuf rec_tab, rec_tabz, rec_tabpre;  // the batched check's shared affine window tables
  DevBuf rec_tab_rows;                   // ... as 224-byte rows (the gather layout; r05l)
  DevBuf rec_wide_tab;                   // a wide group's window tables, one chunk of rounds (rec_tab_wide_layout)
  size_t recw_budget = RECW_TABLE_BUDGET;  // ... and that chunk's byte budget (DGPU_RECOVER_WIDE_BUDGET=<bytes>, A/B)
  bool recover_exact = false;    // DGPU_RECOVER=exact: every round on the per-partial path (A/B)
  size_t cof_engine_max = 16384;  // DGPU_COF_ENGINE_MAX=<rounds>: calls up to this size clear the hash cofactor on
                                 // the engine ladder (k_cof_*; 0 = always k_h2c_finish)
  DevBuf cof_tmp;                // its scratch planes
  bool dec_overlap = true;       // one-lane per-round calls decode on stream2 beside the hash (DGPU_DEC_OVERLAP=0: off)
  bool msm_seg = true;           // load-balanced bucket sums (k_msm_bucket_seg); DGPU_MSM_SEG=0: one thread per bucket (A/B)
  int n_cu = 256;                // compute units (the load-balanced sums launch one wave per SIMD slot)
  bool recover_rows = true;      // the MSM gathers its window tables as rows (DGPU_RECOVER_ROWS=0: SoA planes, A/B)
  // host-record staging: the pinned ring's two slots, their DMA events, the copy stream
  void* ring[2] = {nullptr, nullptr};
  hipEvent_t ring_ev[2] = {nullptr, nullptr};
  bool ring_busy[2] = {false, false};
  int ring_next = 0;
  hipStream_t stream_copy = nullptr;
  float last_stage_ms = 0.f;      // the last host-record call's staging span (dgpu_staging_stats)
  double last_stage_host_ms = 0.0;
  bool test_stage_only = false;   // A/B build, DGPU_TEST_STAGE_ONLY=1: host-record calls stage and stop (staging rehearsal)
  size_t last_stage_bytes = 0;
  bool test_miller_mark = false; // A/B build, DGPU_TEST_MILLER_MARK=1: the six-lane Miller launches get stage marks of their
                                 // own (eng_miller6, eng_miller_tail), so a test can see which kernels a call ran
  bool test_fe_mark = false;     // A/B build, DGPU_TEST_FE_MARK=1: the six-lane FE segment launches get a stage mark of their
                                 // own (eng_fe_seg6)
  bool kb_pair = false;          // A/B: DGPU_KB_PAIR=1, the Karabina chain on two lanes per round (k_kb_chain_pair)
  bool reduce_norm = false;      // A/B: DGPU_REDUCE_NORM=1, k_kb_chain_thr and k_lines_thr with the carried form of
                                 // fp_reduce_lz (fp.cuh; the form before profiles/r15)
  bool lines_wave = false;       // A/B: DGPU_LINES_WAVE=1, k_lines_thr with a pair per wave (G1 point in SGPRs;
                                 // spills 280 -> 226 but 1.5% slower, r06f)
  int eng_xw = 0;                // 16-group 192-thread engine blocks (no idle lanes): bit 0 the Miller loop
                                 // (k_eng_miller_xw), bit 1 the FE segments (k_eng_fe_seg_xw); A/B: DGPU_ENG_XW
  bool stage_pageable = false;   // A/B build, DGPU_STAGE=pageable: the round-5 whole-batch pageable copy
  // staging for host-pointer entry points
  DevBuf in_rounds, in_sigs, in_sig_len, in_prev, in_prev_len, in_msgs, in_msg_len, out_bits, out_reason, out_rand, misc;
  DevBuf in_rows, in_row_ok;    // dgpu_verify_rows: the packed stored rows with their positions and lengths; the decoder's ok flags
  DevBuf in_keys;               // dgpu_check_rows: the rows' keys, staged beside the rows
  DevBuf chk, chk_out;          // the faulty list's scratch (check_rows_layout) and dgpu_check_rows' device lists
  DevBuf in_halo, in_halo_len;  // a staged shard's halo (dgpu_verify_segment_multi): one record of the stride, its length
  // dgpu_verify_keyed: the staged key indices; the key table (keyed_table_layout) and the gathered per-item keys;
  // the pinned copy the table is uploaded from and the event of its last upload
  DevBuf in_key_idx, ky_tab, ky_keys, ky_rlc, ky_exact;  // ... RLC mode: keyed_rlc_layout, keyed_exact_layout
  size_t keyed_range = 0;  // A/B: DGPU_KEYED_RANGE=<entries>, list entries per thread of the per-key sums (0: the default)
  void* ky_host = nullptr;
  size_t ky_host_cap = 0;
  hipEvent_t ky_ev = nullptr;
  bool ky_ev_used = false;
  // optional per-stage HIP-event timing of the last verify call (event pool;
  // durations are summed per stage name: chunked stages repeat)
  bool profile = false;
  std::vector<hipEvent_t> ev;
  std::vector<const char*> stage_name;
  int n_ev = 0;
  bool ev_overflow = false;  // the last call recorded more than STAGE_EVENTS_MAX stage events
  // per-rank RLC protocol (dgpu_rlc_root_device -> the caller's exchange of
  // roots -> dgpu_rlc_finish_device): the shard's points stay in rlc_tree /
  // sig_pts / status between the two calls; any other verify or recovery
  // call on the context cancels the pending root
  bool rlc_pending = false;
  verify_args rlc_args{};
  uint8_t rlc_pk[96] = {};
  size_t rlc_pk_len = 0;
};

namespace {

// Calls on one context are ordered: each entry point makes its stream wait
// for the previous call's work (which may sit on another stream) and records
// `done` when it has enqueued its own, so shared scratch is never
// overwritten mid-flight whatever streams the caller uses.
struct stream_order {
  dgpu_ctx* c;
  hipStream_t s;
  stream_order(dgpu_ctx* c_, hipStream_t s_) : c(c_), s(s_) { (void)hipStreamWaitEvent(s, c->done, 0); }
  ~stream_order() { (void)hipEventRecord(c->done, s); }
};

// N temporary device buffers of a data tool.  However the tool returns, the
// stream that used them is synchronised first (the destructor's body) and the
// buffers, being members, are freed after it.
template <int N>
struct stream_scratch {
  hipStream_t s;
  DevBuf b[N];
  explicit stream_scratch(hipStream_t s_) : s(s_) {}
  ~stream_scratch() { (void)hipStreamSynchronize(s); }
};

// A fork to a side stream (the decode beside the hash, the cofactor's U):
// however the function returns, the main stream ends up waiting for all the
// side stream's work, so the call's `done` event (recorded on the main
// stream) covers it (an early return after the fork left a
// decode running unjoined).  release() once the function has joined itself.
struct side_join {
  hipStream_t side, main;
  hipEvent_t ev;
  bool armed;
  side_join(hipStream_t side_, hipStream_t main_, hipEvent_t ev_) : side(side_), main(main_), ev(ev_), armed(side_ != nullptr) {}
  void release() { armed = false; }
  ~side_join() {
    if (armed && hipEventRecord(ev, side) == hipSuccess) (void)hipStreamWaitEvent(main, ev, 0);
  }
};

// The stream a *_device entry point enqueues on: the caller's, and NULL is
// the device's legacy default (null) stream -- the handle torch's default
// stream has -- never the context's own non-blocking stream.  Until ABI 2
// NULL meant the context's stream, which is unordered with the null stream:
// a caller that zero-filled outputs or read the RLC root on its default
// stream raced the library (gpurun_out/r04c: a rank read its root before the
// MSM wrote it, the all-zero root is the identity, the node check passed and
// a corrupted round was accepted).
hipStream_t caller_stream(void* stream) { return (hipStream_t)stream; }

// Stage markers: mark(c, s, name) records an event that *starts* stage `name`
// (and ends the previous one); mark(c, s, nullptr) closes the last stage.
constexpr int STAGE_EVENTS_MAX = 4096;
void mark(dgpu_ctx* c, hipStream_t s, const char* name = nullptr) {
  if (!c->profile) return;
  if (c->n_ev >= STAGE_EVENTS_MAX) {  // reported by dgpu_stage_times, never dropped silently
    c->ev_overflow = true;
    return;
  }
  if ((size_t)c->n_ev == c->ev.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    c->ev.push_back(e);
    c->stage_name.push_back(nullptr);
  }
  (void)hipEventRecord(c->ev[c->n_ev], s);
  c->stage_name[c->n_ev] = name;
  c->n_ev++;
}

// The start of a verify or recovery call's device work: no stage events yet,
// and a pending per-rank RLC root (dgpu_rlc_root_device) is cancelled.
void call_reset(dgpu_ctx* c) {
  c->n_ev = 0;
  c->ev_overflow = false;
  c->rlc_pending = false;
}

// Engine block constants (slot order of tools/gen_engine.py: ONE, the two
// pairing points (-x, y) -- the key (zero without one) and -g1 --,
// gamma1_1..5, gamma2_1..5).  unit_points: both points (1, 1), for the on-G1
// fixed-line table.  Synchronous upload.
int upload_eng_consts(DevBuf* dst, const g1_key* key, bool unit_points = false) {
  eng_const_block cb;
  memset(&cb, 0, sizeof cb);
  const fp2 g1c[5] = {C_FROB1_1, C_FROB1_2, C_FROB1_3, C_FROB1_4, C_FROB1_5};
  const fp2 g2c[5] = {C_FROB2_1, C_FROB2_2, C_FROB2_3, C_FROB2_4, C_FROB2_5};
  auto put = [&](int slot, const fp& v) { memcpy(cb.w + (slot - 64) * ENG_SLOT_WORDS, v.l, FP_LIMBS * 4); };
  const g1_key zero{fp_zero(), fp_zero()};
  const g1_key& k = key ? *key : zero;
  put(ENG_C_ONE, fp_one());
  put(ENG_C_NXP0, unit_points ? fp_one() : k.neg_x);
  put(ENG_C_YP0, unit_points ? fp_one() : k.y);
  put(ENG_C_NXP1, unit_points ? fp_one() : fp_neg(C_G1_X));
  put(ENG_C_YP1, unit_points ? fp_one() : C_G1_NEG_Y);
  for (int j = 0; j < 5; ++j) {
    put(ENG_C_G1 + 2 * j, g1c[j].c0);
    put(ENG_C_G1 + 2 * j + 1, g1c[j].c1);
    put(ENG_C_G2 + j, g2c[j].c0);
  }
  const fp2 cx = C_PSI_CX, cy = C_PSI_CY;
  put(ENG_C_PSI, cx.c0);
  put(ENG_C_PSI + 1, cx.c1);
  put(ENG_C_PSI + 2, cy.c0);
  put(ENG_C_PSI + 3, cy.c1);
  int rc;
  if ((rc = dst->ensure(sizeof cb))) return rc;
  HIP_TRY(hipMemcpy(dst->p, &cb, sizeof cb, hipMemcpyHostToDevice));
  return DGPU_OK;
}

// Decode a 48-byte G1 key into e (public-key decode of InfoFromProto,
// chain/convert.go:20-23); synchronous on the context's stream.
int decode_g1_key_locked(dgpu_ctx* c, key_entry* e, const uint8_t* pk) {
  g1_key_misc M;
  int rc = carve(c->misc, &M);
  if (rc) return rc;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(M.in, pk, 48, hipMemcpyHostToDevice, s));
  RC_TRY(launch(k_decode_g1_pk, dim3(1), dim3(64), s, M.in, M.out, M.rc));
  uint32_t host[2 * FP_LIMBS + 1];  // out and, next to it, rc
  HIP_TRY(hipMemcpyAsync(host, M.out, sizeof host, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int drc = (int)host[2 * FP_LIMBS];
  if (drc != DEC_OK) return set_err(DGPU_EINVAL, "public key rejected (decode code %d)", drc);
  memcpy(e->pk.neg_x.l, host, FP_LIMBS * 4);
  memcpy(e->pk.y.l, host + FP_LIMBS, FP_LIMBS * 4);
  return upload_eng_consts(&e->consts, &e->pk);
}

// G2 key (on-G1 schemes): decode (subgroup-checked) and compute the fixed-Q
// line table: the LINES program for (pk, g2) at P = (1, 1).
int decode_g2_key_locked(dgpu_ctx* c, key_entry* e, const uint8_t* pk) {
  int rc;
  g2_key_misc M;
  if ((rc = e->table.ensure(eng_blk_words(1, ENG_LINE_STEPS) * 4)) || (rc = carve(c->misc, &M))) return rc;
  if ((rc = upload_eng_consts(&e->consts, nullptr))) return rc;
  DevBuf unit;  // read by k_eng_lines below, which every return path after its launch waits for
  if ((rc = upload_eng_consts(&unit, nullptr, true))) return rc;
  uint32_t *const d_pk = M.pk, *const d_g2 = M.g2;
  int* const d_rc = M.rc;
  uint8_t* const d_in = M.in;
  g2a gen{C_G2_X, C_G2_Y};
  uint32_t gw[G2A_WORDS];
  memcpy(gw, gen.x.c0.l, 56);
  memcpy(gw + 14, gen.x.c1.l, 56);
  memcpy(gw + 28, gen.y.c0.l, 56);
  memcpy(gw + 42, gen.y.c1.l, 56);
  hipStream_t s = c->stream;
  hipError_t err = hipMemcpyAsync(d_in, pk, 96, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipMemcpyAsync(d_g2, gw, sizeof gw, hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return set_err(DGPU_EDEVICE, "set_pubkey: %s", hipGetErrorString(err));
  RC_TRY(launch(k_decode_g2_pk, dim3(1), dim3(64), s, d_in, d_pk, d_rc));
  int drc = -1;
  err = hipMemcpyAsync(&drc, d_rc, sizeof drc, hipMemcpyDeviceToHost, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) return set_err(DGPU_EDEVICE, "set_pubkey: %s", hipGetErrorString(err));
  if (drc != DEC_OK) return set_err(DGPU_EINVAL, "public key rejected (decode code %d)", drc);
  RC_TRY(launch(k_eng_lines, dim3(1), dim3(ENG_BLOCK), s, 1, 0, 1, d_pk, 1, nullptr, d_g2, nullptr, unit.u32(),
                e->table.u32(), nullptr, nullptr));
  err = hipStreamSynchronize(s);
  if (err != hipSuccess) return set_err(DGPU_EDEVICE, "set_pubkey lines: %s", hipGetErrorString(err));
  return DGPU_OK;
}

// The cached key entry for (scheme's key group, pk bytes), decoding it into a
// free or least-recently-used slot on a miss.  Chains, schemes and callers
// can interleave on one context: nothing key-specific lives outside the
// entries.
int get_key_locked(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t len, key_entry** out) {
  if (!pk) return set_err(DGPU_EINVAL, "null public key");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  const bool g2key = sig_on_g1(scheme);
  const size_t want = g2key ? 96 : 48;
  if (len != want)
    return set_err(DGPU_EINVAL, "public key must be %zu bytes (compressed %s), got %zu", want, g2key ? "G2" : "G1", len);
  key_entry* victim = nullptr;
  for (key_entry& e : c->keys) {
    if (e.used && e.g2key == g2key && !memcmp(e.bytes, pk, want)) {
      e.stamp = ++c->clock;
      *out = &e;
      return DGPU_OK;
    }
    if (!victim || (!e.used && victim->used) || (e.used == victim->used && e.stamp < victim->stamp)) victim = &e;
  }
  // the victim's buffers may still be read by an earlier asynchronous call
  HIP_TRY(hipEventSynchronize(c->done));
  if (c->cur == victim) c->cur = nullptr;
  victim->used = false;
  int rc = g2key ? decode_g2_key_locked(c, victim, pk) : decode_g1_key_locked(c, victim, pk);
  if (rc) return rc;
  victim->used = true;
  victim->g2key = g2key;
  memcpy(victim->bytes, pk, want);
  victim->stamp = ++c->clock;
  *out = victim;
  return DGPU_OK;
}

// Karabina final exponentiation of one chunk (pairing_engine.cuh, DESIGN.md
// 2b): segment 0 (easy part), then per exponentiation by |x| the compressed
// chain, its six stored values' norms, the batched inversion of their
// products (divsteps, fp.cuh fp_inv), the decompression, and the next 12-lane
// segment (the split at the inversion -- parts formed at the chain's snaps,
// one thread per round inverting and decompressing -- measured slower, r04j,
// and removed in round 6); last, the Granger-Scott kernel for the listed
// blocks with a flagged item.  capb: the chunk capacity
// rounded up to whole blocks of 5 rounds (>= cnt); kb: the chunk's state,
// carved for capb / 5 blocks.
int eng_fe_kb_locked(dgpu_ctx* c, const uint32_t* consts, size_t cnt, size_t capb, size_t r0, uint32_t* f,
                     const uint32_t* n1inv, const eng_kb_layout& kb, uint8_t* st, hipStream_t s) {
  if (capb % ENG_ROUNDS_PER_BLOCK || cnt > capb) return set_err(DGPU_EINVAL, "karabina FE: bad chunk capacity");
  uint32_t *const xbuf = kb.xbuf, *const pbuf = kb.pbuf, *const pre = kb.pre, *const ebuf = kb.ebuf, *const fb = kb.fb;
  uint8_t* const flags = kb.flags;
  const unsigned blocks = grid_for(cnt, ENG_ROUNDS_PER_BLOCK);
  const size_t inv_threads = std::max<size_t>(1, (cnt + c->kb_inv_chain - 1) / c->kb_inv_chain);
  constexpr int nseg = (int)(sizeof(ENG_PROG_FEK_OFF) / sizeof(ENG_PROG_FEK_OFF[0])) - 1;
  static_assert(nseg == 6, "segment 0 + one per exponentiation by |x|");
  for (int seg = 0; seg < nseg; ++seg) {
    if (seg > 0) {
      mark(c, s, "eng_fe_chain");
      const bool kb_thread = c->kb_thread && cnt >= c->thr_min;
      const bool norm_pre = kb_thread && c->kb_norm_chain;
      if (norm_pre && c->kb_pair)  // two lanes per round
        RC_TRY(launch_n(k_kb_chain_pair<true>, 2 * cnt, 256, s, cnt, xbuf, ebuf));
#ifdef DG_AB_KNOBS
      else if (kb_thread && c->reduce_norm)
        RC_TRY(launch_n(norm_pre ? k_kb_chain_thr<true, false> : k_kb_chain_thr<false, false>, cnt, 256, s, cnt, xbuf,
                        norm_pre ? ebuf : nullptr));
#endif
      else if (kb_thread)
        RC_TRY(launch_n(norm_pre ? k_kb_chain_thr<true> : k_kb_chain_thr<false>, cnt, 256, s, cnt, xbuf,
                        norm_pre ? ebuf : nullptr));
      else
        RC_TRY(launch(k_eng_kb_chain, dim3(grid_for(cnt, 8)), dim3(64), s, cnt, xbuf));
      mark(c, s, "eng_fe_kbinv");
      RC_TRY(launch_n(norm_pre ? k_eng_kb_norm<true> : k_eng_kb_norm<false>, cnt, 256, s, cnt, r0, xbuf, pbuf, ebuf, flags,
                      st, c->kb_test_flag));
      RC_TRY(launch_n(k_eng_inv, inv_threads, 256, s, cnt, r0, pbuf, pre, st));
      RC_TRY(launch_n(k_eng_kb_dec, (size_t)ENG_KB_NSNAP * cnt, 256, s, cnt, xbuf, pbuf, ebuf, flags));
    }
    mark(c, s, "eng_fe");
    const int so = ENG_PROG_FEK_OFF[seg], sl = ENG_PROG_FEK_OFF[seg + 1] - ENG_PROG_FEK_OFF[seg];
    const bool first = seg == 0, last = seg == nseg - 1;
#ifdef DG_AB_KNOBS
    if (c->eng_xw & 2) {  // measured slower too (r06d)
      RC_TRY(launch(first || last ? k_eng_fe_seg_xw<ENG_SLOTS_FE> : k_eng_fe_seg_xw<ENG_FEK_MID_SLOTS>,
                    dim3(grid_for(cnt, ENG_XW_ITEMS)), dim3(ENG_XW_BLOCK), s, so, sl, first, last, cnt, r0, consts, f, n1inv,
                    xbuf, flags, fb, st));
      continue;
    }
#endif
    if (!first && c->feseg6 && cnt >= c->thr_min) {  // segments 1..5 with one Fp2 coefficient per lane
#ifdef DG_AB_KNOBS
      if (c->test_fe_mark) mark(c, s, "eng_fe_seg6");
#endif
      RC_TRY(launch(k_eng_fe_seg6, dim3(grid_for(cnt, M6_ITEMS_PER_WAVE)), dim3(ENG_BLOCK), s, seg, cnt, r0, consts, xbuf,
                    flags, fb, st));
    } else {
      RC_TRY(launch(k_eng_fe_seg, dim3(blocks), dim3(ENG_BLOCK), s, so, sl, first, last, cnt, r0, consts, f, n1inv, xbuf,
                    flags, fb, st));
    }
  }
  return launch(k_eng_fe_fb, dim3(ENG_FB_GRID), dim3(ENG_BLOCK), s, cnt, r0, consts, f, n1inv, st, flags, fb);
}

// One batch of pairing checks for eng_pairing_locked: item i passes when
// e(P_i, h_i) e(-g1, sg_i) == 1 with P_i the key in `consts` or item i's in
// pk_items (G2 signatures), or e(h_i, Q) e(-sg_i, g2) == 1 with Q fixed
// (fixed_table: its line table) or item i's in g1form_keys (G1 signatures).
struct pairing_job {
  const uint32_t* consts = nullptr;  // engine block constants (a key's, or the context's without one)
  size_t n = 0;                      // items
  const uint32_t* h = nullptr;       // hash points, SoA over h_stride items ...
  const uint32_t* sg = nullptr;      // signature points, SoA over n items
  uint8_t* st = nullptr;             // ST_* per item: decode verdicts in, pairing verdicts out
  size_t h_stride = 0;               // ... 0: n
  const uint32_t* h_idx = nullptr;   // item i's hash point index (null: i)
  const uint32_t* pk_items = nullptr;     // a G1 key per item (recovery)
  const uint32_t* fixed_table = nullptr;  // G1 signatures: the key's fixed-Q line table
  lane_scratch* lane = nullptr;           // the lane's engine scratch (null: lane 0)
  bool sig_subgroup = false;              // the lines kernel checks the signatures' G2 membership
  const uint32_t* g1form_keys = nullptr;  // G1 signatures: a G2 key per item (recovery)
};

// Per-round pairing checks on the lane-cooperative engine, chunk by chunk
// (pairing_engine.cuh): lines -> Miller product + norm -> batch inversion ->
// final exponentiation.  Decode verdicts in `st` stay final.
int eng_pairing_locked(dgpu_ctx* c, const pairing_job& job, hipStream_t s) {
  const uint32_t* const consts = job.consts;
  const size_t n = job.n;
  const uint32_t *const h = job.h, *const sg = job.sg;
  uint8_t* const st = job.st;
  const size_t h_stride = job.h_stride ? job.h_stride : n;
  const uint32_t *const h_idx = job.h_idx, *const pk_items = job.pk_items, *const fixed_table = job.fixed_table;
  lane_scratch& L = job.lane ? *job.lane : c->lane[0];
  const bool sig_subgroup = job.sig_subgroup;
  const uint32_t* const g1form_keys = job.g1form_keys;
  const bool need_lines = !(fixed_table && c->fused_fixed);
  // small calls: the Granger-Scott FE (one launch; the Karabina side's five
  // chain / norm / batched-inversion / decompression rounds are latency there)
  const bool fe_gs = c->fe_gs || n <= c->fe_gs_max;
  int rc;
  size_t cap = 0, cap_blk = 0;
  eng_kb_layout kb{};
  bool retried = false;
  for (;;) {
    // equal chunks of at most eng_chunk items (whole 5-item blocks): no short tail launch
    const size_t nchunks = (n + c->eng_chunk - 1) / c->eng_chunk;
    cap = (n + nchunks - 1) / nchunks;
    cap = std::min(n, (cap + ENG_ROUNDS_PER_BLOCK - 1) / ENG_ROUNDS_PER_BLOCK * ENG_ROUNDS_PER_BLOCK);
    cap_blk = eng_blocks(cap);  // blocked layouts
    // the Karabina planes are wave-blocked: whole blocks of 5 rounds (cap may be n, not a multiple of 5)
    rc = fe_gs ? DGPU_OK : carve(L.kb, &kb, cap_blk);
    if (!rc && need_lines) rc = L.lines.ensure(eng_blk_words(cap_blk, ENG_LINE_STEPS) * 4);
    if (!rc) rc = L.f.ensure(eng_blk_words(cap_blk, ENG_F_PLANES) * 4);
    if (!rc) rc = L.n1.ensure(eng_n1_words(cap) * 4);
    if (rc != DGPU_ENOMEM || c->eng_chunk <= ENG_CHUNK_MIN || cap <= ENG_CHUNK_MIN) break;
    // HBM is shared (other contexts, torch): the chunk was sized from the free
    // memory at dgpu_open; halve it for this context and retry.
    // The buffers may still be read by this context's earlier work (its two
    // streams and the call's stream); nothing else has to wait.
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream2));
    for (DevBuf* b : {&L.kb, &L.lines, &L.f, &L.n1}) b->release();
    c->eng_chunk = std::max(ENG_CHUNK_MIN, c->eng_chunk / 2);
    ++c->chunk_retries;
    retried = true;
  }
  if (rc) return rc;
  if (retried) g_last_error.clear();  // the failed attempt's message is stale
  // k_eng_inv's prefix products (eng_n1_words(cap)) reuse the line buffer: they fit
  // in its cap_blk blocks (scratch_layouts.h's static_assert); the fused path has
  // no line buffer and sizes lane 0's for them alone
  uint32_t* lines = need_lines ? L.lines.u32() : nullptr;
  uint32_t* f = L.f.u32();
  uint32_t* n1 = L.n1.u32();
  uint32_t* pre = need_lines ? lines : nullptr;
  if (!pre) {
    if ((rc = c->lane[0].lines.ensure(eng_n1_words(cap) * 4))) return rc;
    pre = c->lane[0].lines.u32();
  }
  uint8_t* const sub_st = sig_subgroup ? st : nullptr;
  for (size_t r0 = 0; r0 < n; r0 += cap) {
    const size_t cnt = std::min(cap, n - r0);
    const dim3 blocks(grid_for(cnt, ENG_ROUNDS_PER_BLOCK)), eng(ENG_BLOCK);
    if (!need_lines) {  // on-G1, lines formed inside the Miller kernel
      mark(c, s, "eng_miller");
      RC_TRY(launch(k_eng_miller_fixed, blocks, eng, s, n, r0, cnt, consts, h, sg, fixed_table, f, n1));
    } else {
      const bool thr = c->lines_thread && cnt >= c->thr_min;
      if (g1form_keys) {  // G1-signature recovery: h and sg affine G1 points, pair 0's G2 point per item
        mark(c, s, "eng_lines");
        RC_TRY(launch_n(k_lines_thr_g1, 2 * cnt, 256, s, n, r0, cnt, h, h_stride, h_idx, sg, g1form_keys, lines));
      } else if (fixed_table) {  // on-G1: h and sg are affine G1 points, the G2 arguments fixed
        mark(c, s, "eng_lines_fixed");
        RC_TRY(launch(k_eng_lines_fixed, dim3(blocks.x, ENG_LINE_STEPS), eng, s, n, r0, cnt, h, sg, fixed_table, lines));
      } else if (thr && !pk_items && c->lines_wave) {  // pair per wave: P in SGPRs
        mark(c, s, "eng_lines");
        RC_TRY(launch_n(k_lines_thr<true>, 2 * ((cnt + 63) / 64 * 64), 256, s, n, r0, cnt, h, h_stride, h_idx, sg, pk_items,
                        consts, lines, sub_st));
      } else if (thr) {
        mark(c, s, "eng_lines");
#ifdef DG_AB_KNOBS
        const auto k = c->reduce_norm ? k_lines_thr<false, false> : k_lines_thr<false>;
#else
        const auto k = k_lines_thr<false>;
#endif
        RC_TRY(launch_n(k, 2 * cnt, 256, s, n, r0, cnt, h, h_stride, h_idx, sg, pk_items, consts, lines, sub_st));
      } else {
        mark(c, s, "eng_lines");
        RC_TRY(launch(k_eng_lines, blocks, eng, s, n, r0, cnt, h, h_stride, h_idx, sg, pk_items, consts, lines, sub_st,
                      nullptr));
      }
      mark(c, s, "eng_miller");
#ifdef DG_AB_KNOBS
      if (c->eng_xw & 1)  // no idle lanes, barrier-ordered: measured 8% slower (profiles/r06/r06d_engine_xw_ab.txt)
        RC_TRY(launch(k_eng_miller_xw, dim3(grid_for(cnt, ENG_XW_ITEMS)), dim3(ENG_XW_BLOCK), s, cnt, consts, lines, f, n1));
      else
#endif
      if (c->miller6 && cnt >= c->thr_min) {  // one Fp2 coefficient per lane, then N1 = Norm(f) from fbuf
#ifdef DG_AB_KNOBS
        if (c->test_miller_mark) mark(c, s, "eng_miller6");
#endif
        RC_TRY(launch(k_eng_miller6, dim3(grid_for(cnt, M6_ITEMS_PER_WAVE)), eng, s, cnt, lines, f));
#ifdef DG_AB_KNOBS
        if (c->test_miller_mark) mark(c, s, "eng_miller_tail");
#endif
        RC_TRY(launch(k_eng_miller_tail, blocks, eng, s, cnt, consts, f, n1));
      } else {
        RC_TRY(launch(k_eng_miller, blocks, eng, s, cnt, consts, lines, f, n1));
      }
    }
    const size_t inv_threads = std::max<size_t>(1, (cnt + 63) / 64);
    mark(c, s, "eng_inv");
    RC_TRY(launch_n(k_eng_inv, inv_threads, 256, s, cnt, r0, n1, pre, st));
    if (fe_gs) {
      mark(c, s, "eng_fe");
      RC_TRY(launch(k_eng_fe, blocks, eng, s, cnt, r0, consts, f, n1, st));
    } else if ((rc = eng_fe_kb_locked(c, consts, cnt, cap_blk * ENG_ROUNDS_PER_BLOCK, r0, f, n1, kb, st, s))) {
      return rc;
    }
  }
  return DGPU_OK;
}

// ---------------------------------------------------------------- RLC
// The segment trees of one RLC batch (level l: P[l], S[l], sz[l] nodes).
using rlc_trees = sum_levels;

// Word sizes of one signature group's points in the RLC buffers.
struct rlc_geom {
  bool g1;
  int aw, jw;  // affine / Jacobian words per point
};
inline rlc_geom rlc_geom_of(bool g1) {
  return with_group(g1, [&](auto gr) { return rlc_geom{g1, GrMem<GROUP_OF(gr)>::AFF, GrMem<GROUP_OF(gr)>::JAC}; });
}

// The SSWU stage of the G2 hash over 2n field elements u -> Jacobian points
// in q: the fused k_h2c_sswu.
int launch_sswu(size_t n, const uint32_t* u, uint32_t* q, hipStream_t s) {
  return launch_n(k_h2c_sswu, 2 * n, 256, s, n, u, q);
}

// rlc_tree of a batch of n rounds: the trees' levels and the points R_i.
// rlc_points_locked allocates it; the later stages of the batch carve the
// same buffer again (same n, same group: nothing is reallocated).
int rlc_tree_carve(dgpu_ctx* c, size_t n, const rlc_geom& G, rlc_tree_layout* t) {
  return carve(c->rlc_tree, t, n, G.aw, G.jw);
}

// RLC phase 1: R_i = pre-cofactor H(m_i) (affine, in rlc_tree's tail),
// sig_i decoded (+ subgroup, required before any combination: soundness --
// both groups' cofactors have small prime factors, so a small-order component
// would survive a random 64-bit combination with noticeable probability).
// Asynchronous on s.
int rlc_points_locked(dgpu_ctx* c, const verify_args& a, hipStream_t s) {
  const unsigned B = 256;
  const size_t n = a.n;
  const rlc_geom G = rlc_geom_of(sig_on_g1(a.scheme));
  int rc;
  lane_scratch& L = c->lane[0];
  rlc_tree_layout tree;
  if ((rc = rlc_tree_carve(c, n, G, &tree))) return rc;
  if ((rc = L.sig_pts.ensure(n * G.aw * 4)) || (rc = L.h_pre.ensure(n * FP_WORDS * 4))) return rc;
  uint32_t* const rpts = tree.rpts;
  uint32_t* sg = L.sig_pts.u32();
  uint8_t* st = c->status.u8();
  if (G.g1) {
    mark(c, s, "rlc_hash_to_g1_raw");
    RC_TRY(with_src(a.m, [&](const auto& m) {
      return launch_n(SRC_KERNEL(k_hash_to_g1_raw, m), n, B, s, n, m, a.scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, rpts,
                      tree.rz);
    }));
    mark(c, s, "decode_g1");
    RC_TRY(with_src(a.m, [&](const auto& m) {
      return launch_n(SRC_KERNEL(k_decode_g1_sigs, m), n, B, s, n, a.sigs, a.sig_stride, a.sig_len, m, sg, st);
    }));
    mark(c, s, "rlc_affine");
    return launch_n(k_g1_batch_affine, (n + 15) / 16, B, s, n, rpts, tree.rz, L.h_pre.u32());
  }
  h2c_tmp_layout tmp;
  if ((rc = carve(L.h_tmp, &tmp, n, false))) return rc;
  mark(c, s, "rlc_hash_to_g2_raw");
  // the per-round hash's field and SSWU stages, then Q0 + Q1 without the cofactor
  RC_TRY(with_src(a.m, [&](const auto& m) { return launch_n(SRC_KERNEL(k_h2c_field, m), n, B, s, n, m, tmp.u); }));
  RC_TRY(launch_sswu(n, tmp.u, tmp.q, s));
  RC_TRY(launch_n(k_h2c_sum, n, B, s, n, tmp.q, rpts));
  mark(c, s, "decode_g2");
  RC_TRY(with_src(a.m, [&](const auto& m) {
    return launch_n(SRC_KERNEL(k_decode_g2_sigs_sub, m), n, B, s, n, a.sigs, a.sig_stride, a.sig_len, m, sg, st);
  }));
  mark(c, s, "rlc_affine");
  // R_i to affine in place (X, Y slots; Z follows them in the Jacobian SoA)
  return launch_n(k_g2_batch_affine, (n + 15) / 16, B, s, n, rpts, tree.rz, L.h_pre.u32());
}

// RLC root by bucket MSM (rlc_msm.cuh) into root (P then S, stride-1
// Jacobian of the signature group).  Asynchronous on s.
template <class Gr>
int rlc_root_msm_t(dgpu_ctx* c, const verify_args& a, hipStream_t s, const rlc_root_layout& root, const char* stage) {
  using M = GrMem<Gr>;
  const unsigned B = 256;
  const size_t n = a.n;
  // list positions and bucket offsets are 32-bit: up to MSM_MW entries per round
  if (n > 0xFFFFFFFFull / MSM_MW) return set_err(DGPU_EINVAL, "RLC batch too large for one MSM (%zu rounds)", n);
  int rc;
  rlc_tree_layout tree;
  msm_counts_layout mc;
  msm_list_layout ml;
  msm_runs_layout mr;
  if ((rc = rlc_tree_carve(c, n, rlc_geom_of(sig_on_g1(a.scheme)), &tree)) ||
      (rc = c->msm_aos.ensure(2 * n * M::AFF * 4)) || (rc = c->msm_flags.ensure(n)) ||
      (rc = carve(c->msm_counts, &mc)) || (rc = carve(c->msm_list, &ml, n)) ||
      (rc = c->msm_buckets.ensure(MSM_KEYS * M::JAC * 4)) || (rc = carve(c->msm_runs, &mr, M::JAC)))
    return rc;
  uint32_t* aos = c->msm_aos.u32();
  uint8_t* flags = c->msm_flags.u8();
  uint32_t *const counts = mc.counts, *const offsets = mc.offsets, *const cursor = mc.cursor;
  uint32_t* const list = ml.list;
  uint32_t* const keys = c->msm_seg ? ml.keys : nullptr;  // the key of every list entry
  // load-balanced sums: 4 SIMDs x 2 resident waves (launch bounds 256, 2) per CU
  const size_t seg_threads = (size_t)c->n_cu * 4 * 2 * 64;
  if (c->msm_seg && (rc = c->msm_part.ensure(2 * seg_threads * M::JAC * 4))) return rc;
  mark(c, s, stage);
  RC_TRY(launch_n(k_msm_aos<Gr>, n, B, s, n, tree.rpts, c->lane[0].sig_pts.u32(), c->status.u8(), aos, flags));
  HIP_TRY(hipMemsetAsync(counts, 0, MSM_KEYS * 4, s));
  RC_TRY(launch_n(k_msm_count, n, B, s, n, a.seed, flags, counts));
  RC_TRY(launch(k_msm_scan, dim3(1), dim3(1024), s, counts, offsets, cursor));
  RC_TRY(launch_n(k_msm_scatter, n, B, s, n, a.seed, flags, cursor, list, keys));
  uint32_t* buckets = c->msm_buckets.u32();
  if (c->msm_seg) {
    uint32_t* part = c->msm_part.u32();
    RC_TRY(launch_n(k_msm_bucket_seg<Gr>, seg_threads, B, s, n, seg_threads, offsets, counts, list, keys, aos, buckets,
                    part));
    RC_TRY(launch_n(k_msm_fixup<Gr>, MSM_KEYS, B, s, seg_threads, offsets, counts, part, buckets));
  } else {
    RC_TRY(launch_n(k_msm_bucket<Gr>, MSM_KEYS, B, s, n, offsets, counts, list, aos, buckets));
  }
  uint32_t *runs = mr.runs, *runs2 = mr.runs2;
  RC_TRY(launch_n(k_msm_window<Gr>, (size_t)MSM_MW * MSM_RUNS, B, s, buckets, runs));
  size_t len = MSM_RUNS;
  while (len > 1) {  // pairwise tree per (MSM, window), ping-pong between the two run buffers
    const size_t nl = (len + 1) / 2;
    RC_TRY(launch_n(k_sum_level<Gr>, (size_t)MSM_MW * nl, B, s, MSM_MW, len, runs, nl, runs2));
    std::swap(runs, runs2);
    len = nl;
  }
  return launch(k_msm_root<Gr>, dim3(1), dim3(64), s, runs, root.P, root.S);
}

// The root goes to `dst` (rlc_root_layout: P then S).
int rlc_root_msm_locked(dgpu_ctx* c, const verify_args& a, hipStream_t s, DevBuf& dst, rlc_root_layout* out = nullptr,
                        const char* stage = "rlc_root_msm") {
  rlc_root_layout root;
  int rc = carve(dst, &root, rlc_geom_of(sig_on_g1(a.scheme)).jw);
  if (rc) return rc;
  if (out) *out = root;
  return with_group(sig_on_g1(a.scheme), [&](auto gr) { return rlc_root_msm_t<GROUP_OF(gr)>(c, a, s, root, stage); });
}

// The segment trees of one RLC batch (leaves P_i = r_i R_i, S_i = r_i sig_i,
// r_i from the seed and the batch position i; then sums up to the root),
// built from rlc_points_locked's points.  Asynchronous on s.
template <class Gr>
int rlc_tree_t(dgpu_ctx* c, const verify_args& a, hipStream_t s, rlc_trees& T, bool plain) {
  const unsigned B = 256;
  const size_t n = a.n;
  rlc_tree_layout tree;
  int rc = rlc_tree_carve(c, n, rlc_geom_of(sig_on_g1(a.scheme)), &tree);
  if (rc) return rc;
  T = tree.T;
  mark(c, s, plain ? "rlc_plain_tree" : "rlc_leaves_tree");
  const uint32_t* const sg = c->lane[0].sig_pts.u32();
  const uint8_t* const st = c->status.u8();
  if (plain)
    RC_TRY(launch_n(k_rlc_leaves_plain<Gr>, 2 * n, B, s, n, tree.rpts, sg, st, T.P[0], T.S[0]));
  else
    RC_TRY(launch_n(k_rlc_leaves<Gr>, 2 * n, B, s, n, a.seed, tree.rpts, sg, st, T.P[0], T.S[0]));
  for (int l = 0; l < T.top(); ++l)
    RC_TRY(launch_n(k_rlc_level<Gr>, 2 * T.sz[l + 1], B, s, T.sz[l], T.P[l], T.S[l], T.sz[l + 1], T.P[l + 1], T.S[l + 1]));
  return DGPU_OK;
}

int rlc_tree_locked(dgpu_ctx* c, const verify_args& a, hipStream_t s, rlc_trees& T, bool plain = false) {
  return with_group(sig_on_g1(a.scheme), [&](auto gr) { return rlc_tree_t<GROUP_OF(gr)>(c, a, s, T, plain); });
}

// The identity (Z = 0) of the signature group as a stride-1 Jacobian point
// (jw words): the root of an empty shard.
int rlc_identity_words(bool g1, uint32_t* w) {
  const g2j inf2 = g2_infinity();
  const g1j inf1 = g1_infinity();
  const fp* co2[6] = {&inf2.x.c0, &inf2.x.c1, &inf2.y.c0, &inf2.y.c1, &inf2.z.c0, &inf2.z.c1};
  const fp* co1[3] = {&inf1.x, &inf1.y, &inf1.z};
  const int nc = g1 ? 3 : 6;
  for (int j = 0; j < nc; ++j) memcpy(w + j * FP_LIMBS, (g1 ? co1[j] : co2[j])->l, FP_LIMBS * 4);
  return nc * FP_LIMBS;
}

// Check candidate nodes cand of a level (P_lvl, S_lvl, n_level nodes) on the
// pairing engine: e(pk, h_eff P) e(-g1, S) == 1 (G2 signatures) or
// e(h_eff P, pk) e(-S, g2) == 1 (G1 signatures: the key's fixed-Q line
// table).  Fail flags stay on the device (d_fail, one byte per candidate);
// `fail` (optional) receives them on the host (synchronizes the stream).
int rlc_check_locked(dgpu_ctx* c, const key_entry* key, const std::vector<uint32_t>& cand, size_t n_level,
                     const uint32_t* P_lvl, const uint32_t* S_lvl, hipStream_t s, std::vector<uint8_t>* fail) {
  const unsigned B = 256;
  const size_t m = cand.size();
  const rlc_geom G = rlc_geom_of(key->g2key);
  int rc;
  if ((rc = c->rlc_idx.ensure(m * 4)) || (rc = c->rlc_fail.ensure(m))) return rc;
  if ((rc = c->rlc_h.ensure(m * G.aw * 4)) || (rc = c->rlc_s.ensure(m * G.aw * 4)) || (rc = c->rlc_st.ensure(m)))
    return rc;
  uint32_t* d_idx = c->rlc_idx.u32();
  uint8_t* d_fail = c->rlc_fail.u8();
  HIP_TRY(hipMemcpyAsync(d_idx, cand.data(), m * 4, hipMemcpyHostToDevice, s));
  uint32_t* ch = c->rlc_h.u32();
  uint32_t* cs = c->rlc_s.u32();
  uint8_t* cst = c->rlc_st.u8();
  mark(c, s, "rlc_prep");
  RC_TRY(with_group(G.g1, [&](auto gr) {
    return launch_n(k_rlc_prep<GROUP_OF(gr)>, m, 64, s, m, d_idx, n_level, P_lvl, S_lvl, ch, cs, cst);
  }));
  if ((rc = eng_pairing_locked(c,
                               {.consts = key->consts.u32(),
                                .n = m,
                                .h = ch,
                                .sg = cs,
                                .st = cst,
                                .fixed_table = G.g1 ? key->table.u32() : nullptr},
                               s)))
    return rc;
  mark(c, s, "rlc_bisection");
  RC_TRY(launch_n(k_rlc_fail, m, B, s, m, cst, d_fail));
  if (fail) {
    fail->resize(m);
    HIP_TRY(hipMemcpyAsync(fail->data(), d_fail, m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DGPU_OK;
}

// RLC phase 2, root first: the whole batch is one node check (one final
// exponentiation) when every round is valid.  Otherwise the wide descent:
// check every node of the level with <= 64Ki nodes (a multiple of D levels,
// DGPU_RLC_DESCENT_STEP, default 3,
// up from the leaves), then all descendants D levels down of each failing
// node, to the leaves; a failing leaf is an invalid round (ST_PAIRING).
int rlc_descend_locked(dgpu_ctx* c, const key_entry* key, const rlc_trees& T, hipStream_t s,
                       bool root_failed = false, std::vector<uint32_t>* leaf_cand = nullptr) {
  const unsigned B = 256;
  const int D = c->rlc_descent_step;
  const int top = T.top();
  uint8_t* st = c->status.u8();
  std::vector<uint8_t> fail;
  std::vector<uint32_t> cand{0};
  mark(c, s, "rlc_bisection");
  if (top > 0 && !root_failed) {
    int rc = rlc_check_locked(c, key, cand, 1, T.P[top], T.S[top], s, &fail);
    if (rc) return rc;
    if (!fail[0]) return DGPU_OK;  // every decodable round verifies
  }
  int S0 = 0;
  while (S0 + D <= top && T.sz[S0] > 65536) S0 += D;
  if (T.sz[S0] > 65536 && S0 < top) S0 = top;
  int l = S0;
  if (S0 == top && top > 0) {  // the root failed: its descendants D levels down
    l = top >= D ? top - D : 0;
    cand.clear();
    for (size_t j = 0; j < T.sz[l]; ++j) cand.push_back((uint32_t)j);
  } else {
    cand.resize(T.sz[S0]);
    for (size_t j = 0; j < T.sz[S0]; ++j) cand[j] = (uint32_t)j;
  }
  while (!cand.empty()) {
    int rc = rlc_check_locked(c, key, cand, T.sz[l], T.P[l], T.S[l], s, l == 0 ? nullptr : &fail);
    if (rc) return rc;
    if (l == 0) {
      RC_TRY(launch_n(k_rlc_mark, cand.size(), B, s, cand.size(), c->rlc_idx.u32(), c->rlc_fail.u8(), st));
      if (leaf_cand) leaf_cand->swap(cand);  // rlc_idx / rlc_fail still hold them on the device
      break;
    }
    const int nl = l >= D ? l - D : 0;
    const size_t span = (size_t)1 << (l - nl);
    std::vector<uint32_t> next;
    for (size_t k = 0; k < cand.size(); ++k) {
      if (!fail[k]) continue;
      const size_t lo = (size_t)cand[k] * span, hi = std::min(lo + span, T.sz[nl]);
      for (size_t j = lo; j < hi; ++j) next.push_back((uint32_t)j);
    }
    cand.swap(next);
    l = nl;
  }
  return DGPU_OK;
}

// RLC phase 2 when a root containing this shard failed: exact per-round
// verdicts (DESIGN.md 2c "localize, then confirm").  shard_root: this
// shard's random-combination root (stride-1 P, S; seed a.seed).
//  0. Unless it is known failing (root_failed: it was the node's root), the
//     shard's own root is checked first: passing, the shard is valid.
//  1. Localize on the tree of plain sums (coefficients 1, k_rlc_leaves_plain):
//     its leaves cost nothing (the points themselves) and a leaf check is the
//     round's own pairing check, so every round it marks ST_PAIRING is
//     exactly invalid.  Bad rounds can hide only in an internal node whose
//     errors cancel in the plain sum (crafted input).
//  2. Confirm the rest: the shard's root minus the marked rounds' terms (their
//     random-coefficient leaves, a few per thousand rounds), one check.  It
//     passes for a correct localization; then every remaining round is valid
//     except with probability 2^-64 -- the coefficients are uniform and
//     independent of the localization, which uses plain sums only.
//  3. Only if the confirmation fails: the random-coefficient tree (leaves
//     [a] R + [b] endo(R)) over what is left, descended as before.
template <class Gr>
int rlc_confirm_t(dgpu_ctx* c, const key_entry* key, const verify_args& a, hipStream_t s,
                  const rlc_root_layout& shard_root, const std::vector<uint32_t>& leaf_cand, bool* ok) {
  using M = GrMem<Gr>;
  const unsigned B = 256;
  int rc;
  mark(c, s, "rlc_confirm");
  const size_t mc = leaf_cand.size();
  rlc_conf_layout cf;
  rlc_tree_layout tree;
  if ((rc = carve(c->rlc_conf, &cf, mc, M::JAC)) ||
      (rc = rlc_tree_carve(c, a.n, rlc_geom_of(sig_on_g1(a.scheme)), &tree)))
    return rc;
  const rlc_root_layout& conf = cf.root;  // confirmation root
  uint32_t *const count = cf.count, *const list = cf.list;
  uint32_t nf = 0;
  if (mc) {
    HIP_TRY(hipMemsetAsync(count, 0, 4, s));
    RC_TRY(launch_n(k_rlc_compact_fail, mc, B, s, mc, c->rlc_idx.u32(), c->rlc_fail.u8(), list, count));
    HIP_TRY(hipMemcpyAsync(&nf, count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (nf) {  // the marked rounds' leaves, summed pairwise to one (P, S)
    sum_levels F;
    if ((rc = carve(c->rlc_fsum, &F, (size_t)nf, M::JAC))) return rc;
    RC_TRY(launch_n(k_rlc_leaves_list<Gr>, 2 * (size_t)nf, B, s, nf, list, a.n, a.seed, tree.rpts,
                    c->lane[0].sig_pts.u32(), F.P[0], F.S[0]));
    for (int l = 0; l < F.top(); ++l)
      RC_TRY(launch_n(k_rlc_level<Gr>, 2 * F.sz[l + 1], B, s, F.sz[l], F.P[l], F.S[l], F.sz[l + 1], F.P[l + 1], F.S[l + 1]));
    // (one node: stride 1; the kernel reads the shard's root and writes conf as P | S)
    RC_TRY(launch(k_rlc_sub_root<Gr>, dim3(1), dim3(64), s, shard_root.P, F.P[F.top()], F.S[F.top()], conf.P));
  } else {
    HIP_TRY(hipMemcpyAsync(conf.P, shard_root.P, layout_bytes<rlc_root_layout>(M::JAC), hipMemcpyDeviceToDevice, s));
  }
  std::vector<uint8_t> fail;
  if ((rc = rlc_check_locked(c, key, std::vector<uint32_t>{0}, 1, conf.P, conf.S, s, &fail))) return rc;
  *ok = !fail[0];
  return DGPU_OK;
}

int rlc_resolve_locked(dgpu_ctx* c, const key_entry* key, const verify_args& a, hipStream_t s,
                       const rlc_root_layout& shard_root, bool root_failed) {
  int rc;
  const bool g1 = sig_on_g1(a.scheme);
  if (!root_failed) {
    std::vector<uint8_t> fail;
    if ((rc = rlc_check_locked(c, key, std::vector<uint32_t>{0}, 1, shard_root.P, shard_root.S, s, &fail))) return rc;
    if (!fail[0]) return DGPU_OK;
  }
  rlc_trees T;
  if (c->rlc_localize) {
    std::vector<uint32_t> leaf_cand;
    if ((rc = rlc_tree_locked(c, a, s, T, true)) || (rc = rlc_descend_locked(c, key, T, s, true, &leaf_cand)))
      return rc;
    bool ok = false;
    rc = with_group(g1, [&](auto gr) { return rlc_confirm_t<GROUP_OF(gr)>(c, key, a, s, shard_root, leaf_cand, &ok); });
    if (rc || ok) return rc;
  }
  if ((rc = rlc_tree_locked(c, a, s, T))) return rc;
  return rlc_descend_locked(c, key, T, s, true);
}

// Per-round G1 path, first half (the counterpart of g2_lane_hash_locked):
// H(m) in G1, batch affine and the G1 signature decode of a's records into
// lane 0's buffers.  side: the decode runs on stream2 beside the hash (as the
// G2 path's s_dec); s waits for it before returning.
int g1_hash_decode_locked(dgpu_ctx* c, const verify_args& a, uint8_t* st, hipStream_t s, bool side) {
  const unsigned B = 256;
  const size_t n = a.n;
  int rc;
  lane_scratch& L = c->lane[0];
  if ((rc = L.h_pts.ensure(n * 2 * FP_WORDS * 4)) || (rc = L.sig_pts.ensure(n * 2 * FP_WORDS * 4)) ||
      (rc = L.h_z.ensure(n * FP_WORDS * 4)) || (rc = L.h_pre.ensure(n * FP_WORDS * 4)))
    return rc;
  uint32_t* h = L.h_pts.u32();
  auto decode = [&](hipStream_t sd) {
    return with_src(a.m, [&](const auto& m) {
      return launch_n(SRC_KERNEL(k_decode_g1_sigs, m), n, B, sd, n, a.sigs, a.sig_stride, a.sig_len, m, L.sig_pts.u32(),
                      st);
    });
  };
  side_join join(side ? c->stream2 : nullptr, s, c->lane_ev[1]);
  if (side) {
    RC_TRY(stream_after(c->stream2, s, c->lane_ev[0]));
    RC_TRY(decode(c->stream2));
    HIP_TRY(hipEventRecord(c->lane_ev[1], c->stream2));
  }
  mark(c, s, "hash_to_g1");
  RC_TRY(with_src(a.m, [&](const auto& m) {
    return launch_n(SRC_KERNEL(k_hash_to_g1_beacons, m), n, B, s, n, m, a.scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, h,
                    L.h_z.u32());
  }));
  mark(c, s, "h_affine");
  RC_TRY(launch_n(k_g1_batch_affine, (n + 15) / 16, B, s, n, h, L.h_z.u32(), L.h_pre.u32()));
  if (side) {
    HIP_TRY(hipStreamWaitEvent(s, c->lane_ev[1], 0));
    join.release();
    return DGPU_OK;
  }
  mark(c, s, "decode_g1");
  return decode(s);
}

// Signatures on G1: the front half above (the decode beside the hash on the
// second stream), then the engine's Miller (fixed-Q lines) / inversion /
// final-exponentiation kernels.
int verify_g1_locked(dgpu_ctx* c, const key_entry* key, const verify_args& a, uint8_t* st, hipStream_t s) {
  int rc = g1_hash_decode_locked(c, a, st, s, c->dec_overlap && c->lanes > 1 && !c->profile);
  if (rc) return rc;
  const lane_scratch& L = c->lane[0];
  return eng_pairing_locked(c,
                            {.consts = key->consts.u32(),
                             .n = a.n,
                             .h = L.h_pts.u32(),
                             .sg = L.sig_pts.u32(),
                             .st = st,
                             .fixed_table = key->table.u32()},
                            s);
}

// host-record staging (verify_status_host_locked): the kernels of a slice
// wait for its records
struct host_stager;
int stager_wait_msg(host_stager* stg, size_t k, hipStream_t s);
int stager_wait_sig(host_stager* stg, size_t k, hipStream_t s);
int stager_wait_all(host_stager* stg, hipStream_t s);

// Per-round G2 path, first half of one lane: hash-to-G2 (field, SSWU, finish),
// batch affine, signature decode of `n` items into the lane's buffers.
// s_dec (optional): the signature decode runs on that stream, beside the hash
// chain on s (it reads only the records and writes sig_pts and the statuses);
// s waits for it before returning.
// decode_sub: the decoder checks the signatures' G2 membership whatever the
// context's setting (a caller that combines the points before any lines kernel).
// consts (the key's engine constants; optional): calls of at most
// cof_engine_max rounds clear the cofactor on the engine ladder
// (pairing_engine.cuh k_cof_*) instead of k_h2c_finish.
int g2_lane_hash_locked(dgpu_ctx* c, lane_scratch& L, size_t n, const msg_src_host& m, const uint8_t* sigs,
                        size_t sig_stride, const uint32_t* sig_len, uint8_t* st, hipStream_t s,
                        hipStream_t s_dec = nullptr, const uint32_t* consts = nullptr, host_stager* stg = nullptr,
                        size_t slice = 0, bool decode_sub = false) {
  const unsigned B = 256;
  int rc;
  h2c_tmp_layout tmp;  // u, q, then k_h2c_finish's park region and its redo flags
  if ((rc = L.h_pts.ensure(n * G2A_WORDS * 4)) || (rc = L.sig_pts.ensure(n * G2A_WORDS * 4)) ||
      (rc = L.h_z.ensure(n * 2 * FP_WORDS * 4)) || (rc = L.h_pre.ensure(n * FP_WORDS * 4)) ||
      (rc = carve(L.h_tmp, &tmp, n, true)))
    return rc;
  uint32_t *const h = L.h_pts.u32(), *const sg = L.sig_pts.u32(), *const hz = L.h_z.u32();
  uint32_t *const u = tmp.u, *const q = tmp.q, *const park = tmp.park;
  uint8_t* const redo = tmp.redo;
  // membership of the signature: checked by the lines kernel (eng_pairing_locked sig_subgroup)
  auto decode = [&](hipStream_t sd) {
    return with_src(m, [&](const auto& ms) {
      if (c->decode_subgroup || decode_sub)
        return launch_n(SRC_KERNEL(k_decode_g2_sigs_sub, ms), n, B, sd, n, sigs, sig_stride, sig_len, ms, sg, st);
      return launch_n(SRC_KERNEL(k_decode_g2_sigs, ms), n, B, sd, n, sigs, sig_stride, sig_len, ms, 0, sg, st);
    });
  };
  const bool cof_engine = consts && n <= c->cof_engine_max;
  const unsigned cof_blocks = grid_for(n, ENG_ROUNDS_PER_BLOCK);
  cof_tmp_layout cof{};
  if (cof_engine && ((rc = carve(c->cof_tmp, &cof, n)) ||
                     (rc = L.lines.ensure(eng_blk_words(cof_blocks, ENG_LINE_STEPS) * 4))))
    return rc;  // allocated before the fork: a failure here leaves nothing on the side stream
  side_join join(s_dec, s, c->lane_ev[1]);
  if (s_dec) {  // first in the second stream's queue: it runs beside the whole hash chain
    RC_TRY(stream_after(s_dec, s, c->lane_ev[0]));
    if ((rc = stager_wait_sig(stg, slice, s_dec))) return rc;  // host records: the slice's signatures on the device
    RC_TRY(decode(s_dec));
    HIP_TRY(hipEventRecord(c->lane_ev[1], s_dec));
  }
  mark(c, s, "hash_to_g2");
  RC_TRY(with_src(m, [&](const auto& ms) { return launch_n(SRC_KERNEL(k_h2c_field, ms), n, B, s, n, ms, u); }));
  RC_TRY(launch_sswu(n, u, q, s));
  if (cof_engine) {
    const dim3 blocks(cof_blocks), eng(ENG_BLOCK);
    // (the k_cof_* kernels take the planes' base and address them by COF_* themselves)
    uint32_t *const w = cof.pj, *const pa = cof.pa, *const psia = cof.psia, *const t1 = cof.t1, *const t0a = cof.t0a,
                    *const t2 = cof.t2;
    uint32_t* lines = L.lines.u32();
    RC_TRY(launch_n(k_cof_prep, n, B, s, n, q, w));
    RC_TRY(launch(k_eng_lines, blocks, eng, s, n, 0, n, pa, n, nullptr, psia, nullptr, consts, lines, nullptr, t1));
    RC_TRY(launch_n(k_cof_mid, n, B, s, n, w));
    // U (everything but [x^2]P) on the second stream beside the second pass
    const bool side = s_dec != nullptr;
    const hipStream_t su = side ? s_dec : s;
    if (side) RC_TRY(stream_after(su, s, c->cof_ev[0]));
    RC_TRY(launch_n(k_cof_partial, n, B, su, n, w));
    if (side) HIP_TRY(hipEventRecord(c->cof_ev[1], su));
    RC_TRY(launch(k_eng_lines, blocks, eng, s, n, 0, n, t0a, n, nullptr, t0a, nullptr, consts, lines, nullptr, t2));
    if (side) HIP_TRY(hipStreamWaitEvent(s, c->cof_ev[1], 0));
    RC_TRY(launch_n(k_cof_final, n, B, s, n, w, h, hz));
  } else {
    RC_TRY(launch_n(k_h2c_finish, n, B, s, n, q, park, redo, h, hz));
    RC_TRY(launch_n(k_h2c_finish_redo, n, B, s, n, redo, park, h, hz));
  }
  mark(c, s, "h_affine");
  RC_TRY(launch_n(k_g2_batch_affine, (n + 15) / 16, B, s, n, h, hz, L.h_pre.u32()));
  if (s_dec) {
    HIP_TRY(hipStreamWaitEvent(s, c->lane_ev[1], 0));  // the decode (queued first on s_dec)
    join.release();
    return DGPU_OK;
  }
  mark(c, s, "decode_g2");
  if ((rc = stager_wait_sig(stg, slice, s))) return rc;
  return decode(s);
}

// msg_src of items [off, off + cnt) of m.  The linked form keeps its base
// pointers (the slice's first item reads the record before the slice) and
// carries the offset.
msg_src_host src_slice(const msg_src_host& m, size_t off) {
  msg_src_host r = m;
  if (m.linked) {
    r.g0 = m.g0 + off;
  } else if (m.msgs) {
    r.msgs = m.msgs + off * m.msg_stride;
    r.msg_len = m.msg_len + off;
  } else {
    r.rounds = m.rounds + off;
    if (m.chained) {
      r.prev = m.prev + off * m.prev_stride;
      r.prev_len = m.prev_len + off;
    }
  }
  return r;
}

// The stored rows of a row call (verify_args' m.rows).  The caller's rows
// (row i = len[i] bytes at base + off[i]) are staged packed back to back:
// slen[i] is the staged length (len[i], or 0 for a row longer than any
// canonical row at the strides: it is non-canonical whatever it holds and is
// not staged), pos[i] row i's position in the packed run (pos[n] = the run's
// bytes).  The device side (rows_prepare_locked): the packed run and the two
// arrays (in_rows), and the record arrays k_ingest_rows writes -- the
// context's in_* buffers, the verify call's inputs.
struct rows_src {
  const uint8_t* base;
  const uint64_t* off;
  const uint32_t* len;
  std::vector<uint32_t> slen;
  std::vector<uint64_t> pos;
  ingest_rows_layout dev;
  uint64_t* d_rounds;
  uint8_t *d_sigs, *d_prev, *d_ok;
  uint32_t *d_sig_len, *d_prev_len;
  size_t sig_stride, prev_stride;
  // dgpu_check_rows: the rows' keys (host), staged slice by slice behind the
  // slice's rows into d_keys; nullptr for dgpu_verify_rows
  const uint64_t* keys;
  uint64_t* d_keys;
};

// The host side of a rows_src: the caller's arrays and the strides.
rows_src rows_src_of(const uint8_t* base, const uint64_t* row_off, const uint32_t* row_len, const uint64_t* keys,
                     size_t sig_stride, size_t prev_stride) {
  rows_src R{};
  R.base = base, R.off = row_off, R.len = row_len, R.keys = keys;
  R.sig_stride = sig_stride, R.prev_stride = prev_stride;
  return R;
}

// The argument checks of a row call with rows: the row arrays and the strides.
int rows_check_args(const rows_src& R, size_t sig_bytes) {
  if (!R.base || !R.off || !R.len) return set_err(DGPU_EINVAL, "null row or output buffer");
  if (R.sig_stride < sig_bytes) return set_err(DGPU_EINVAL, "bad signature stride");
  const size_t max_len = ingest_row_max_len(R.sig_stride, R.prev_stride);
  if (R.sig_stride > STAGE_SLOT_BYTES || R.prev_stride > STAGE_SLOT_BYTES || max_len + 16 > STAGE_SLOT_BYTES)
    return set_err(DGPU_EINVAL, "strides too large for the staging ring");
  return DGPU_OK;
}

int check_args(const dgpu_ctx* c, const key_entry* key, const verify_args& a) {
  if (!scheme_known(a.scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", a.scheme);
  if (a.mode != DGPU_MODE_PER_ROUND && a.mode != DGPU_MODE_RLC) return set_err(DGPU_EINVAL, "bad mode %d", a.mode);
  if (!key) return set_err(DGPU_ENOKEY, "no public key installed (dgpu_set_pubkey)");
  if (sig_on_g1(a.scheme) != key->g2key)
    return set_err(DGPU_ENOKEY, "the public key is on the wrong group for scheme %d", a.scheme);
  if (a.n == 0) return DGPU_OK;
  const size_t sig_bytes = sig_on_g1(a.scheme) ? 48 : 96;
  if (a.m.rows) return rows_check_args(*a.m.rows, sig_bytes);  // (the record buffers are the context's)
  if (!a.sigs || !a.sig_len || a.sig_stride < sig_bytes) return set_err(DGPU_EINVAL, "bad signature buffers");
  if (a.m.msgs || a.m.msg_len) {
    if (!a.m.msgs || !a.m.msg_len) return set_err(DGPU_EINVAL, "bad message buffers");
  } else if (!a.m.linked) {  // (the linked form's records are the signature arrays, checked above)
    if (!a.m.rounds) return set_err(DGPU_EINVAL, "null rounds");
    if (a.m.chained && (!a.m.prev_len || (!a.m.prev && a.m.prev_stride)))
      return set_err(DGPU_EINVAL, "chained scheme needs previous signatures");
  }
  (void)c;
  return DGPU_OK;
}

// Rounds per slice of the per-round G2 path's lanes (verify_status_locked),
// which host-record staging follows; the whole batch for every other pipeline.
size_t lane_slice_len(const dgpu_ctx* c, const verify_args& a) {
  const size_t n = a.n;
  if ((a.mode == DGPU_MODE_RLC && n >= c->rlc_min) || sig_on_g1(a.scheme)) return std::max<size_t>(n, 1);
  const bool two = c->lanes > 1 && !c->profile && n >= LANE_MIN;
  const size_t slices = two ? std::max<size_t>(2, c->lane_slices) : 1;
  return two ? ((n / slices + ENG_ROUNDS_PER_BLOCK - 1) / ENG_ROUNDS_PER_BLOCK) * ENG_ROUNDS_PER_BLOCK
             : std::max<size_t>(n, 1);
}


// Everything up to the per-item status (ST_*): G1 or G2 signatures, per-round
// or RLC.  Asynchronous on s (RLC descent synchronizes between its levels).
// stg (host records, verify_status_host_locked): each slice's kernels wait
// for that slice's staging.
int verify_status_locked(dgpu_ctx* c, const key_entry* key, const verify_args& a, hipStream_t s,
                         host_stager* stg = nullptr) {
  const size_t n = a.n;
  int rc;
  if ((rc = c->status.ensure(n))) return rc;
  uint8_t* st = c->status.u8();
  call_reset(c);
  if (a.mode == DGPU_MODE_RLC && n >= c->rlc_min) {
    // root first, by bucket MSM; the tree of leaves only when it fails
    if ((rc = stager_wait_all(stg, s)) || (rc = rlc_points_locked(c, a, s))) return rc;
    rlc_root_layout root;
    if ((rc = rlc_root_msm_locked(c, a, s, c->rlc_root, &root))) return rc;
    std::vector<uint8_t> fail;
    if ((rc = rlc_check_locked(c, key, std::vector<uint32_t>{0}, 1, root.P, root.S, s, &fail))) return rc;
    if (!fail[0] || a.n == 1) {
      if (fail[0])  // one round: its leaf is the root
        RC_TRY(launch(k_rlc_mark, dim3(1), dim3(64), s, 1, c->rlc_idx.u32(), c->rlc_fail.u8(), st));
      return DGPU_OK;
    }
    return rlc_resolve_locked(c, key, a, s, root, true);
  }
  if (sig_on_g1(a.scheme)) return (rc = stager_wait_all(stg, s)) ? rc : verify_g1_locked(c, key, a, st, s);
  const uint32_t* consts = key->consts.u32();
  lane_scratch &L0 = c->lane[0], &L1 = c->lane[1];
  // Two lanes (streams) on the two halves of the batch once it spans more
  // than one engine chunk; lane 1 starts when lane 0's hash/decode kernels
  // are done, so its register-bound hash runs beside lane 0's LDS-bound
  // engine.  Profiled passes stay on one stream (clean per-kernel times).
  const bool two = c->lanes > 1 && !c->profile && n >= LANE_MIN;
  const size_t n0 = two ? lane_slice_len(c, a) : n;
  // one lane: the decode overlaps the hash on the second stream (small calls:
  // the decode's ~0.9 ms leaves the critical path; DGPU_DEC_OVERLAP=0 off)
  // (DGPU_LANES=1 keeps the whole call on one stream: no decode beside the hash either)
  const hipStream_t s_dec = (!two && c->lanes > 1 && c->dec_overlap && !c->profile) ? c->stream2 : nullptr;
  if ((rc = stager_wait_msg(stg, 0, s)) ||
      (rc = g2_lane_hash_locked(c, L0, n0, a.m, a.sigs, a.sig_stride, a.sig_len, st, s, s_dec, consts, stg, 0)))
    return rc;
  const bool sub = !c->decode_subgroup;
  // one slice of the batch on one lane's buffers
  auto slice_job = [&](lane_scratch& L, size_t cnt, uint8_t* sst) {
    return pairing_job{.consts = consts,
                       .n = cnt,
                       .h = L.h_pts.u32(),
                       .sg = L.sig_pts.u32(),
                       .st = sst,
                       .lane = &L,
                       .sig_subgroup = sub};
  };
  if (!two) return eng_pairing_locked(c, slice_job(L0, n, st), s);
  hipStream_t s2 = c->stream2;
  RC_TRY(stream_after(s2, s, c->lane_ev[0]));
  if ((rc = eng_pairing_locked(c, slice_job(L0, n0, st), s))) return rc;
  // the remaining slices alternate between the lanes (stream order keeps each
  // lane's buffers in use by one slice at a time), so a slice's hash runs
  // beside the other lane's engine chunks (DGPU_LANE_SLICES, default 2)
  lane_scratch* LL[2] = {&L0, &L1};
  hipStream_t ss[2] = {s, s2};
  size_t k = 1;
  for (size_t off = n0; off < n; off += n0, ++k) {
    const size_t nk = std::min(n0, n - off);
    const int ln = (int)(k & 1);
    if ((rc = stager_wait_msg(stg, k, ss[ln])) ||
        (rc = g2_lane_hash_locked(c, *LL[ln], nk, src_slice(a.m, off), a.sigs + off * a.sig_stride, a.sig_stride,
                                  a.sig_len + off, st + off, ss[ln], nullptr, nullptr, stg, k)))
      return rc;
    if ((rc = eng_pairing_locked(c, slice_job(*LL[ln], nk, st + off), ss[ln]))) return rc;
  }
  return stream_after(s, s2, c->lane_ev[1]);
}

// ---------------------------------------------------------------- the RLC shard protocol
// The per-rank entry points and multi_verify run these three steps, the exchange of roots between the first two.
// Shard root: the shard's points and its root by bucket MSM, left in msm_root
// and copied to d_root (device; rlc_root_layout); an empty shard's is the identity pair.
int rlc_shard_root_locked(dgpu_ctx* c, const verify_args& a, uint8_t* d_root, hipStream_t s) {
  const rlc_geom G = rlc_geom_of(sig_on_g1(a.scheme));
  if (a.n == 0) {
    uint32_t inf[G2J_WORDS];
    rlc_identity_words(G.g1, inf);
    const rlc_root_layout root = layout_at<rlc_root_layout>(d_root, G.jw);
    HIP_TRY(hipMemcpyAsync(root.P, inf, (size_t)G.jw * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(root.S, inf, (size_t)G.jw * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the host source goes out of scope
    return DGPU_OK;
  }
  rlc_root_layout root;
  int rc;
  if ((rc = c->status.ensure(a.n))) return rc;
  call_reset(c);  // (the callers cancelled a pending root before they staged anything)
  if ((rc = rlc_points_locked(c, a, s)) || (rc = rlc_root_msm_locked(c, a, s, c->msm_root, &root))) return rc;
  HIP_TRY(hipMemcpyAsync(d_root, root.P, layout_bytes<rlc_root_layout>(G.jw), hipMemcpyDeviceToDevice, s));
  return DGPU_OK;
}

// Node check: the n_roots roots at d_roots summed into the context's rlc_root, one
// pairing check of the sum.  *fail: the node's batch holds a bad round.  Synchronizes s.
int rlc_node_check_locked(dgpu_ctx* c, const key_entry* key, size_t n_roots, const uint8_t* d_roots, hipStream_t s,
                          bool* fail) {
  rlc_root_layout sum;
  int rc = carve(c->rlc_root, &sum, rlc_geom_of(key->g2key).jw);
  if (rc) return rc;
  mark(c, s, "rlc_root_sum");
  RC_TRY(with_group(key->g2key, [&](auto gr) {
    return launch(k_rlc_sum_roots<GROUP_OF(gr)>, dim3(1), dim3(64), s, (int)n_roots, (const uint32_t*)d_roots, sum.P, sum.S);
  }));
  std::vector<uint8_t> f;
  if ((rc = rlc_check_locked(c, key, std::vector<uint32_t>{0}, 1, sum.P, sum.S, s, &f))) return rc;
  *fail = f[0] != 0;
  return DGPU_OK;
}

// Shard finish: under a failing node the shard is resolved against its own root in
// msm_root, checked first unless it is the node's (one root: known to fail).
int rlc_shard_finish_locked(dgpu_ctx* c, const key_entry* key, const verify_args& a, bool node_failed, size_t n_roots,
                            hipStream_t s) {
  if (!node_failed || a.n == 0) return DGPU_OK;
  rlc_root_layout shard;
  int rc = carve(c->msm_root, &shard, rlc_geom_of(key->g2key).jw);
  return rc ? rc : rlc_resolve_locked(c, key, a, s, shard, n_roots == 1);
}

// The final statuses -> verdict bitmap, then (d_rand: optional, 32 bytes per
// round) the verified rounds' randomness.  a's signature arrays are device
// memory.  Closes the call's stage markers.
int pack_results_locked(dgpu_ctx* c, const verify_args& a, uint8_t* d_bits, uint8_t* d_rand, hipStream_t s) {
  const unsigned B = 256;
  const uint8_t* st = c->status.u8();
  mark(c, s, "pack_verdicts");
  RC_TRY(launch_n(k_pack_verdicts, (a.n + 7) / 8, B, s, a.n, st, d_bits));
  if (d_rand) {
    mark(c, s, "randomness");
    RC_TRY(launch_n(k_randomness, a.n, B, s, a.n, a.sigs, a.sig_stride, a.sig_len, st, d_rand));
  }
  mark(c, s);
  return DGPU_OK;
}

// status -> verdict bitmap, optional reasons and randomness (device buffers)
int verify_device_locked(dgpu_ctx* c, const key_entry* key, const verify_args& a, uint8_t* d_bits,
                         uint8_t* d_reason, hipStream_t s, uint8_t* d_rand = nullptr) {
  int rc = check_args(c, key, a);
  if (rc || a.n == 0) return rc;
  if (!d_bits) return set_err(DGPU_EINVAL, "null verdict buffer");
  if ((rc = verify_status_locked(c, key, a, s)) || (rc = pack_results_locked(c, a, d_bits, d_rand, s))) return rc;
  if (d_reason) HIP_TRY(hipMemcpyAsync(d_reason, c->status.p, a.n, hipMemcpyDeviceToDevice, s));
  return DGPU_OK;
}

// The context buffer behind a record array (record_arrays.h REC_*).
DevBuf& record_buf(dgpu_ctx* c, int buf) {
  DevBuf* const b[REC_BUFS] = {&c->in_rounds, &c->in_prev,    &c->in_prev_len, &c->in_msgs,    &c->in_msg_len,
                               &c->in_sigs,   &c->in_sig_len, &c->in_halo,     &c->in_halo_len};
  return *b[buf];
}

// The device buffers of the record arrays L of call a; a's pointers become
// the device copies' (their contents: stage_inputs_locked, host_stager).
int record_buffers_locked(dgpu_ctx* c, verify_args& a, const record_list& L) {
  for (const record_array& e : L) {
    DevBuf& b = record_buf(c, e.buf);
    int rc = b.ensure((e.part == PART_ONCE ? 1 : a.n) * e.item_bytes + e.pad);
    if (rc) return rc;
    record_ptr_set(a, e, b.p);
  }
  record_aliases(a);
  return DGPU_OK;
}

// A record of items [lo, hi) longer than its stride fails the host call (the device paths flag it per item).
int record_lengths_check(const record_list& L, int part, size_t lo, size_t hi) {
  size_t i = 0;
  const record_array* e = record_bad_length(L, part, lo, hi, &i);
  return e ? set_err(DGPU_EINVAL, e->len_fmt, i, e->len[i]) : DGPU_OK;
}
// ... of one length array of n items (the data tools' entry points)
int lengths_check(const uint32_t* len, size_t n, size_t stride, const char* fmt) {
  const size_t i = first_long_item(len, 0, n, stride);
  return i < n ? set_err(DGPU_EINVAL, fmt, i, len[i]) : DGPU_OK;
}

// The host records of a verify call into the context's input buffers by whole-batch pageable
// copies (the A/B build's DGPU_STAGE=pageable); a's pointers become the device copies'.
int stage_inputs_locked(dgpu_ctx* c, verify_args& a, hipStream_t s) {
  const verify_args host = a;
  const record_list L = record_arrays(host);
  int rc;
  if ((rc = record_lengths_check(L, PART_MSG, 0, a.n)) || (rc = record_buffers_locked(c, a, L))) return rc;
  for (const record_array& e : L) {
    const size_t bytes = (e.part == PART_ONCE ? 1 : a.n) * e.item_bytes;
    if (bytes) HIP_TRY(hipMemcpyAsync((void*)record_ptr(a, e), record_ptr(host, e), bytes, hipMemcpyHostToDevice, s));
  }
  return DGPU_OK;
}

// ---------------------------------------------------------------- host-record staging
// dgpu_verify_beacons / dgpu_verify_recovered / dgpu_verify_multi take host
// records (the Go caller's slices).  They move through a
// library-owned pinned ring -- two slots per context, filled by a process-wide
// pool of host threads and DMA'd to the device on the context's copy stream,
// a slot reused once its DMA has finished -- slice by slice in the order the
// per-round pipeline consumes them: the hash of slice k starts as soon as
// slice k is on the device, while slice k + 1 is still being copied
// (the lanes of verify_status_locked are the slices).  Pageable
// hipMemcpyAsync copied the whole batch before the first kernel (VERDICT r05
// item 4).

// The pool of host threads that fills the slots: copy_pool.h (host-only).
copy_pool& host_copy_pool() {
  static copy_pool pool(STAGE_COPY_THREADS);
  return pool;
}

// The pinned ring: bytes at src (host) -> dst (device) through the slots, on
// the copy stream, in SLOT-sized pieces (asynchronous; the caller's buffer may
// be reused once this returns -- every piece has been copied into a slot).
int ring_copy_locked(dgpu_ctx* c, void* dst, const void* src, size_t bytes) {
  for (size_t off = 0; off < bytes; off += STAGE_SLOT_BYTES) {
    const size_t len = std::min(STAGE_SLOT_BYTES, bytes - off);
    const int k = c->ring_next;
    c->ring_next ^= 1;
    if (c->ring_busy[k]) HIP_TRY(hipEventSynchronize(c->ring_ev[k]));  // its previous DMA has read the slot
    host_copy_pool().copy(c->ring[k], (const uint8_t*)src + off, len);
    HIP_TRY(hipMemcpyAsync((uint8_t*)dst + off, c->ring[k], len, hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(hipEventRecord(c->ring_ev[k], c->stream_copy));
    c->ring_busy[k] = true;
  }
  return DGPU_OK;
}

// The ring bytes of rows [a, b) of a rows_src: the packed rows, then (on an
// 8-byte boundary) their positions and their lengths.
inline size_t rows_piece_bytes(const rows_src& R, size_t a, size_t b) {
  return (((size_t)(R.pos[b] - R.pos[a]) + 7) & ~(size_t)7) + (b - a) * 12;
}

// Rows [a, b) of a rows_src, on the copy stream: cut by bytes into pieces of
// whole rows, each piece the longest run whose ring bytes (rows_piece_bytes)
// fit one slot; the pool's threads gather a piece's rows into the slot, its
// three parts are DMA'd to in_rows, and k_ingest_rows decodes the piece into
// its rows of the record arrays right behind its DMA.
int ring_rows_locked(dgpu_ctx* c, const rows_src& R, size_t a, size_t b) {
  while (a < b) {
    size_t e = a + 1;  // (one row always fits: checked by the entry point)
    {  // the last e in (a, b] with rows_piece_bytes(a, e) <= the slot: the bytes grow with e
      size_t lo = a + 1, hi = b;
      while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (rows_piece_bytes(R, a, mid) <= STAGE_SLOT_BYTES) lo = mid;
        else hi = mid - 1;
      }
      e = lo;
    }
    const size_t m = e - a, pb = (size_t)(R.pos[e] - R.pos[a]), at_off = (pb + 7) & ~(size_t)7, at_len = at_off + m * 8;
    const int k = c->ring_next;
    c->ring_next ^= 1;
    if (c->ring_busy[k]) HIP_TRY(hipEventSynchronize(c->ring_ev[k]));  // its previous DMA has read the slot
    uint8_t* slot = (uint8_t*)c->ring[k];
    host_copy_pool().gather(slot, R.base, R.off + a, R.slen.data() + a, R.pos.data() + a, m);
    memcpy(slot + at_off, R.pos.data() + a, m * 8);
    memcpy(slot + at_len, R.slen.data() + a, m * 4);
    if (pb) HIP_TRY(hipMemcpyAsync(R.dev.bytes + R.pos[a], slot, pb, hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(hipMemcpyAsync(R.dev.off + a, slot + at_off, m * 8, hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(hipMemcpyAsync(R.dev.len + a, slot + at_len, m * 4, hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(hipEventRecord(c->ring_ev[k], c->stream_copy));
    c->ring_busy[k] = true;
    // the piece's rows lie in [0, pos[e]) of the packed run: nothing behind it is on the device yet
    RC_TRY(launch_n(k_ingest_rows, m, INGEST_ROWS_PER_WAVE, c->stream_copy, m, R.dev.bytes, R.pos[e], R.dev.off + a,
                    R.dev.len + a, R.d_rounds + a, R.d_sigs + a * R.sig_stride, R.sig_stride, R.d_sig_len + a,
                    R.d_prev + a * R.prev_stride, R.prev_stride, R.d_prev_len + a, R.d_ok + a));
    a = e;
  }
  return DGPU_OK;
}

int ring_ensure_locked(dgpu_ctx* c) {
  for (int k = 0; k < 2; ++k) {
    if (c->ring[k]) continue;
    HIP_TRY(hipHostMalloc(&c->ring[k], STAGE_SLOT_BYTES, hipHostMallocDefault));
  }
  if (!c->stream_copy) HIP_TRY(hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k)
    if (!c->ring_ev[k]) HIP_TRY(hipEventCreateWithFlags(&c->ring_ev[k], hipEventDisableTiming));
  return DGPU_OK;
}

// One call's staging: the device buffers for all n records are allocated up
// front (a's pointers rewritten to them); a host thread fills slice after
// slice through the ring.  A slice's message part (rounds, previous
// signatures, or raw messages) goes first -- the hash chain's first kernel
// reads only that -- and its signatures after (the decode runs after the
// hash), each part ending in an event on the copy stream: the first kernel
// waits for half the slice's bytes.  The thread also checks each slice's
// record lengths against their strides (a bad record fails the call with
// DGPU_EINVAL, as before, without a serial pass over the batch in front of
// the first kernel).  wait_msg / wait_sig (k, s) make stream s wait for a
// part (the host first waits until the thread has enqueued it).  The
// destructor joins the thread: nothing of the call's host buffers is read
// after the entry point returns.
struct host_stager {
  dgpu_ctx* c;
  verify_args host;               // the caller's pointers (m.rows: the records are decoded on the device from them)
  record_list list;               // the arrays it stages (record_arrays of `host`)
  std::vector<size_t> lo;         // slice k = [lo[k], lo[k + 1])
  std::vector<hipEvent_t> ev_msg, ev_sig;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  size_t staged_msg = 0, staged = 0;  // parts enqueued (message parts, whole slices)
  int rc = DGPU_OK;
  std::string err;
  std::atomic<bool> cancel{false};
  hipEvent_t t0 = nullptr, t1 = nullptr;  // copy-stream span of the staging (dgpu_staging_stats)
  size_t bytes = 0;
  double host_ms = 0.0;                    // the thread's wall time, first memcpy to last DMA enqueued

  host_stager(dgpu_ctx* c_, const verify_args& h) : c(c_), host(h), list(record_arrays(host)) {}
  ~host_stager() {
    const bool ok = th.joinable();
    cancel = true;
    if (ok) th.join();
    // the staging's span on the copy stream, first piece to last DMA: the
    // host memcpy into the ring paces the DMAs, so this is the staging time
    float ms = 0.f;
    if (ok && rc == DGPU_OK && hipEventSynchronize(t1) == hipSuccess && hipEventElapsedTime(&ms, t0, t1) == hipSuccess) {
      c->last_stage_ms = ms;
      c->last_stage_host_ms = host_ms;
      c->last_stage_bytes = bytes;
    }
    for (auto* v : {&ev_msg, &ev_sig})
      for (hipEvent_t e : *v)
        if (e) (void)hipEventDestroy(e);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
  }
  int make_events(size_t slices) {
    for (auto* v : {&ev_msg, &ev_sig}) {
      v->assign(slices, nullptr);
      for (hipEvent_t& e : *v) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreate(&t0));
    HIP_TRY(hipEventCreate(&t1));
    return DGPU_OK;
  }
  // one part of the list for items [a, b), through the ring (PART_ONCE: the call's one record)
  int copy_part(const verify_args& dev, int part, size_t a, size_t b) {
    for (const record_array& e : list) {
      if (e.part != part) continue;
      const size_t off = part == PART_ONCE ? 0 : a * e.item_bytes, len = (part == PART_ONCE ? 1 : b - a) * e.item_bytes;
      int r = ring_copy_locked(c, (uint8_t*)record_ptr(dev, e) + off, record_ptr(host, e) + off, len);
      if (r) return r;
    }
    return DGPU_OK;
  }
  // Slice k = items [a, b) on the in-order copy stream: the once-per-call entries ahead of
  // everything else of the call (a shard's halo: every event a kernel waits for covers it),
  // the message part (its lengths checked first) and its event, the signature part and its event.
  int stage_slice(const verify_args& dev, size_t k, size_t a, size_t b) {
    const rows_src* rows = host.m.rows;
    const size_t n = b - a;
    int r;
    if (rows) {
      // Stored rows: the slice's rows and their decode, then both events -- the
      // records of slice k exist once its k_ingest_rows launches have run.
      // Staged bytes: the staged rows and 12 bytes (position, length) per row.
      // dgpu_check_rows: the slice's keys behind them, 8 bytes per row.
      if ((r = ring_rows_locked(c, *rows, a, b))) return r;
      bytes += (size_t)(rows->pos[b] - rows->pos[a]) + n * 12;
      if (rows->keys) {
        if ((r = ring_copy_locked(c, rows->d_keys + a, rows->keys + a, n * 8))) return r;
        bytes += n * 8;
      }
    } else if ((r = record_lengths_check(list, PART_MSG, a, b)) || (k == 0 && (r = copy_part(dev, PART_ONCE, a, b))) ||
               (r = copy_part(dev, PART_MSG, a, b))) {
      return r;
    }
    HIP_TRY(hipEventRecord(ev_msg[k], c->stream_copy));
    {
      std::lock_guard<std::mutex> lk(mu);
      staged_msg = k + 1;
    }
    cv.notify_all();
    if (!rows && (r = copy_part(dev, PART_SIG, a, b))) return r;
    if (!rows) bytes += n * record_item_bytes(list);
    HIP_TRY(hipEventRecord(ev_sig[k], c->stream_copy));
    return DGPU_OK;
  }
  void start(const verify_args& dev) {
    th = std::thread([this, dev] {
      (void)hipSetDevice(c->device);
      const auto w0 = std::chrono::steady_clock::now();
      (void)hipEventRecord(t0, c->stream_copy);
      for (size_t k = 0; k + 1 < lo.size(); ++k) {
        int r = cancel ? set_err(DGPU_EINVAL, "staging cancelled") : stage_slice(dev, k, lo[k], lo[k + 1]);
        if (!r && k + 2 == lo.size() && hipEventRecord(t1, c->stream_copy) != hipSuccess)
          r = set_err(DGPU_EDEVICE, "hipEventRecord");
        if (k + 2 == lo.size())
          host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        std::lock_guard<std::mutex> lk(mu);
        if (r) {
          rc = r;
          err = g_last_error;
        } else {
          staged = k + 1;
        }
        cv.notify_all();
        if (r) return;
      }
    });
  }
  int wait_part(size_t k, hipStream_t s, bool sig) {
    // A linked slice has no message part of its own: a chained one hashes its
    // signatures (and the last record of slice k - 1, which the in-order copy
    // stream put on the device before slice k's event); an unchained one
    // hashes nothing that is staged.
    if (host.m.linked && !sig) {
      if (!host.m.chained) return DGPU_OK;
      sig = true;
    }
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return (sig ? staged : staged_msg) > k || rc != DGPU_OK; });
    if ((sig ? staged : staged_msg) <= k) return set_err(rc, "%s", err.c_str());
    HIP_TRY(hipStreamWaitEvent(s, (sig ? ev_sig : ev_msg)[k], 0));
    return DGPU_OK;
  }
  int wait_all(hipStream_t s) { return lo.size() > 1 ? wait_part(lo.size() - 2, s, true) : DGPU_OK; }
};

int stager_wait_msg(host_stager* stg, size_t k, hipStream_t s) { return stg ? stg->wait_part(k, s, false) : DGPU_OK; }
int stager_wait_sig(host_stager* stg, size_t k, hipStream_t s) { return stg ? stg->wait_part(k, s, true) : DGPU_OK; }
int stager_wait_all(host_stager* stg, hipStream_t s) { return stg ? stg->wait_all(s) : DGPU_OK; }

// The device buffers of a staged call; a's pointers become the device
// copies' (their contents arrive slice by slice).
int stage_prepare_locked(dgpu_ctx* c, verify_args& a) {
  int rc = ring_ensure_locked(c);
  return rc ? rc : record_buffers_locked(c, a, record_arrays(a));
}

// The rest of a row call's rows_src behind stage_prepare_locked: staged lengths, packed positions,
// the packed rows on the device and the record arrays the decoder writes (the context's in_* buffers).
int rows_prepare_locked(dgpu_ctx* c, const verify_args& a) {
  rows_src* rows = a.m.rows;
  const size_t max_len = ingest_row_max_len(rows->sig_stride, rows->prev_stride);
  rows->slen.resize(a.n);
  rows->pos.resize(a.n + 1);
  uint64_t at = 0;
  for (size_t i = 0; i < a.n; ++i) {
    rows->slen[i] = rows->len[i] <= max_len ? rows->len[i] : 0;
    rows->pos[i] = at;
    at += rows->slen[i];
  }
  rows->pos[a.n] = at;
  int rc;
  // the decoder writes every row's previous signature, whatever the scheme reads
  if ((rc = c->in_prev.ensure(a.n * rows->prev_stride + 1)) || (rc = c->in_prev_len.ensure(a.n * 4)) ||
      (rc = c->in_row_ok.ensure(a.n)) || (rc = carve(c->in_rows, &rows->dev, (size_t)rows->pos[a.n], a.n)))
    return rc;
  if (rows->keys && (rc = c->in_keys.ensure(a.n * 8))) return rc;
  rows->d_rounds = c->in_rounds.u64();
  rows->d_sigs = c->in_sigs.u8();
  rows->d_sig_len = c->in_sig_len.u32();
  rows->d_prev = c->in_prev.u8();
  rows->d_prev_len = c->in_prev_len.u32();
  rows->d_ok = c->in_row_ok.u8();
  rows->d_keys = rows->keys ? c->in_keys.u64() : nullptr;
  return DGPU_OK;
}

// The front of every staged host call: the device buffers (a's pointers become theirs; a row
// call's records are decoded into them, slice by slice behind their DMA), the copy stream behind
// the previous call, slices of slice_len items with their events, and the staging thread running.
int stager_begin_locked(dgpu_ctx* c, host_stager& stg, verify_args& a, size_t slice_len) {
  int rc;
  if ((rc = stage_prepare_locked(c, a))) return rc;
  if (a.m.rows && (rc = rows_prepare_locked(c, a))) return rc;
  // the copy stream (device buffers, ring slots) after the previous call's work
  HIP_TRY(hipStreamWaitEvent(c->stream_copy, c->done, 0));
  for (size_t off = 0; off < a.n; off += slice_len) stg.lo.push_back(off);
  stg.lo.push_back(a.n);
  if ((rc = stg.make_events(stg.lo.size() - 1))) return rc;
  stg.start(a);
  return DGPU_OK;
}

// verify_status_locked over host records, overlapping their staging with the
// verification: the slices are the per-round G2 path's lane slices
// (lane_slice_len), one slice for every other pipeline.
int verify_status_host_locked(dgpu_ctx* c, const key_entry* key, verify_args& a, hipStream_t s) {
  host_stager stg(c, a);
  int rc = stager_begin_locked(c, stg, a, lane_slice_len(c, a));
  if (rc) return rc;
#ifdef DG_AB_KNOBS
  if (c->test_stage_only) return stg.wait_all(s);  // staging rehearsal: no verification (statuses undefined)
#endif
  rc = verify_status_locked(c, key, a, s, &stg);
  if (!rc) rc = stg.wait_all(s);  // every slice consumed (no-op when the pipeline waited for each)
  return rc;
}

// Every record of a host call on the device before anything else runs on s
// (the RLC root's points need the whole shard): one slice through the ring.
int stage_all_host_locked(dgpu_ctx* c, verify_args& a, hipStream_t s) {
  host_stager stg(c, a);
  int rc = stager_begin_locked(c, stg, a, std::max<size_t>(a.n, 1));
  return rc ? rc : stg.wait_all(s);
}

// The results of a call whose statuses are final, asynchronous on s: the bitmap packed
// (pack_results_locked: stage markers closed) into d_bits -- the context's out_bits when NULL --
// and copied to `bits` (host; optional); the reasons (optional), a copy of the statuses of kind
// `reason_kind` (to the host, or a device buffer); the randomness (optional, host) through out_rand.
int results_out_locked(dgpu_ctx* c, const verify_args& a, uint8_t* d_bits, uint8_t* bits, uint8_t* reason,
                       hipMemcpyKind reason_kind, uint8_t* rand32, hipStream_t s) {
  int rc;
  if (!d_bits) {
    if ((rc = c->out_bits.ensure((a.n + 7) / 8))) return rc;
    d_bits = c->out_bits.u8();
  }
  if (rand32 && (rc = c->out_rand.ensure(a.n * 32))) return rc;
  if ((rc = pack_results_locked(c, a, d_bits, rand32 ? c->out_rand.u8() : nullptr, s))) return rc;
  if (bits) HIP_TRY(hipMemcpyAsync(bits, d_bits, (a.n + 7) / 8, hipMemcpyDeviceToHost, s));
  if (reason) HIP_TRY(hipMemcpyAsync(reason, c->status.p, a.n, reason_kind, s));
  if (rand32) HIP_TRY(hipMemcpyAsync(rand32, c->out_rand.p, a.n * 32, hipMemcpyDeviceToHost, s));
  return DGPU_OK;
}

// Host-buffer verify: stage, verify, copy the verdicts back (synchronous).
// rand32 (optional, n x 32 bytes): the verified rounds' randomness, returned
// with the verdicts.
int verify_host_locked(dgpu_ctx* c, const key_entry* key, verify_args a, uint8_t* verdict_bits, uint8_t* reason,
                       uint8_t* rand32 = nullptr) {
  int rc = check_args(c, key, a);
  if (rc || a.n == 0) return rc;
  if (!verdict_bits) return set_err(DGPU_EINVAL, "null verdict buffer");
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  // (a's pointers are the device copies from here on; DGPU_STAGE=pageable, A/B build: the pre-ring path)
  if (c->stage_pageable) rc = (rc = stage_inputs_locked(c, a, s)) ? rc : verify_status_locked(c, key, a, s);
  else rc = verify_status_host_locked(c, key, a, s);
  if (rc || (rc = results_out_locked(c, a, nullptr, verdict_bits, reason, hipMemcpyDeviceToHost, rand32, s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

// dgpu_verify_rows: verify_host_locked with the records decoded on the device
// from the caller's stored rows (a.m.rows); the decoder's ok flags and rounds
// come back with the verdicts.
int verify_rows_locked(dgpu_ctx* c, const key_entry* key, verify_args a, uint64_t* rounds_out, uint8_t* row_ok,
                       uint8_t* verdict_bits, uint8_t* reason) {
  int rc = check_args(c, key, a);
  if (rc || a.n == 0) return rc;
  if (!row_ok || !verdict_bits) return set_err(DGPU_EINVAL, "null row or output buffer");
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  if ((rc = verify_status_host_locked(c, key, a, s)) ||
      (rc = results_out_locked(c, a, nullptr, verdict_bits, reason, hipMemcpyDeviceToHost, nullptr, s)))
    return rc;
  const rows_src& R = *a.m.rows;
  HIP_TRY(hipMemcpyAsync(row_ok, R.d_ok, a.n, hipMemcpyDeviceToHost, s));
  if (rounds_out) HIP_TRY(hipMemcpyAsync(rounds_out, R.d_rounds, a.n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

// ---------------------------------------------------------------- the faulty list (check_rows.cuh)
// The arguments every form of the faulty-list stage shares: first + count
// must not wrap, and the map's and the grid's index widths bound n and count.
int check_range_args(uint64_t first, size_t count, size_t n) {
  if ((uint64_t)count > UINT64_MAX - first) return set_err(DGPU_EINVAL, "first + count overflows 64 bits");
  if (n >= (size_t)CHECK_NO_ROW) return set_err(DGPU_EINVAL, "too many rows");
  if (count > (size_t)0x7fffffff * CHECK_BLOCK) return set_err(DGPU_EINVAL, "too many visited rounds");
  return DGPU_OK;
}

// dgpu_faulty_rounds_device's kernels on s (count > 0; arguments checked).
int faulty_rounds_locked(dgpu_ctx* c, uint64_t first, size_t count, size_t n, const uint64_t* d_keys,
                         const uint8_t* d_row_ok, const uint64_t* d_rounds, const uint8_t* d_status,
                         uint64_t* d_faulty_pos, uint64_t* d_faulty_val, size_t faulty_cap, uint64_t* d_left_rows,
                         size_t left_cap, uint64_t* d_counts, hipStream_t s) {
  check_rows_layout L;
  int rc = carve(c->chk, &L, count);
  if (rc) return rc;
  const size_t nblk = check_blocks(count);
  HIP_TRY(hipMemsetAsync(L.map, 0xFF, count * 4, s));  // CHECK_NO_ROW everywhere
  const dim3 blocks((unsigned)nblk), B(CHECK_BLOCK);
  if (n) RC_TRY(launch_n(k_check_map, n, CHECK_BLOCK, s, first, count, n, d_keys, L.map));
  RC_TRY(launch(k_check_classify, blocks, B, s, first, count, n, L.map, d_row_ok, d_rounds, d_status, L.flags,
                L.blk_faulty, L.blk_left));
  RC_TRY(launch(k_check_scan, dim3(1), B, s, nblk, L.blk_faulty, L.blk_left, d_counts));
  return launch(k_check_scatter, blocks, B, s, first, count, n, L.map, d_row_ok, d_rounds, d_status, L.flags, L.blk_faulty,
                L.blk_left, d_faulty_pos, d_faulty_val, faulty_cap, d_left_rows, left_cap);
}

// The lists of one context on the host: the totals, and the entries below the caps.
struct check_lists {
  uint64_t n_faulty = 0, n_left = 0;
  std::vector<uint64_t> pos, val, left;
};

// The faulty list of positions [first, first + count) over the n rows the
// context has just verified (keys at d_keys; the decoder's ok flags and rounds;
// the final statuses), behind that work on s; the totals come back first, then
// the entries there are, so the bytes copied follow the faults, not n.
// Synchronises s.
int check_lists_locked(dgpu_ctx* c, uint64_t first, size_t count, size_t n, const uint64_t* d_keys,
                       size_t faulty_cap, size_t left_cap, check_lists& out, hipStream_t s) {
  out = check_lists{};
  if (count == 0) return DGPU_OK;
  faulty_cap = std::min(faulty_cap, count);  // (no more entries than positions, or rows)
  left_cap = std::min(left_cap, n);
  check_lists_layout D;
  int rc = carve(c->chk_out, &D, faulty_cap, left_cap);
  if (rc) return rc;
  if ((rc = faulty_rounds_locked(c, first, count, n, d_keys, c->in_row_ok.u8(), c->in_rounds.u64(), c->status.u8(),
                                 D.faulty_pos, D.faulty_val, faulty_cap, D.left_rows, left_cap, D.counts, s)))
    return rc;
  uint64_t counts[2];
  HIP_TRY(hipMemcpyAsync(counts, D.counts, sizeof counts, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  out.n_faulty = counts[0], out.n_left = counts[1];
  const size_t nf = (size_t)std::min<uint64_t>(counts[0], faulty_cap);
  const size_t nl = (size_t)std::min<uint64_t>(counts[1], left_cap);
  out.pos.resize(nf), out.val.resize(nf), out.left.resize(nl);
  if (nf) {
    HIP_TRY(hipMemcpyAsync(out.pos.data(), D.faulty_pos, nf * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out.val.data(), D.faulty_val, nf * 8, hipMemcpyDeviceToHost, s));
  }
  if (nl) HIP_TRY(hipMemcpyAsync(out.left.data(), D.left_rows, nl * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

// The host-side argument checks of dgpu_check_rows and its _multi form, before
// any device work.
int check_rows_args(size_t n, const uint8_t* base, const uint64_t* row_off, const uint32_t* row_len,
                    const uint64_t* keys, uint64_t first, size_t count, const uint64_t* faulty_pos,
                    const uint64_t* faulty_val, size_t faulty_cap, const uint64_t* n_faulty, const uint64_t* left_rows,
                    size_t left_cap, const uint64_t* n_left) {
  int rc = check_range_args(first, count, n);
  if (rc) return rc;
  if (!n_faulty || !n_left) return set_err(DGPU_EINVAL, "null count output");
  if (n && (!base || !row_off || !row_len || !keys)) return set_err(DGPU_EINVAL, "null row buffer");
  if ((faulty_cap && (!faulty_pos || !faulty_val)) || (left_cap && !left_rows))
    return set_err(DGPU_EINVAL, "null list buffer");
  for (size_t i = 0; i < n; ++i) {
    if (i && keys[i] <= keys[i - 1]) return set_err(DGPU_EINVAL, "keys[%zu] is not above keys[%zu]", i, i - 1);
    uint64_t j;
    if (!check_rows_slot(first, count, keys[i], &j))
      return set_err(DGPU_EINVAL, "keys[%zu] lies outside [first, first + count)", i);
  }
  return DGPU_OK;
}

// dgpu_check_rows on one context (arguments checked by check_rows_args; the
// rows and their keys: a.m.rows).
int check_rows_locked(dgpu_ctx* c, const key_entry* key, verify_args a, uint64_t first, size_t count,
                      size_t faulty_cap, size_t left_cap, check_lists& out, uint8_t* reason) {
  int rc = check_args(c, key, a);
  if (rc) return rc;
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  if (a.n && (rc = verify_status_host_locked(c, key, a, s))) return rc;
  if (a.n) mark(c, s);
  if ((rc = check_lists_locked(c, first, count, a.n, a.m.rows->d_keys, faulty_cap, left_cap, out, s))) return rc;
  if (reason && a.n) {
    HIP_TRY(hipMemcpyAsync(reason, c->status.p, a.n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return DGPU_OK;
}

// The lists into the caller's buffers (entries below the caps; the totals always).
void check_lists_store(const check_lists& L, uint64_t* faulty_pos, uint64_t* faulty_val, size_t faulty_cap,
                       uint64_t* n_faulty, uint64_t* left_rows, size_t left_cap, uint64_t* n_left) {
  const size_t nf = std::min(L.pos.size(), faulty_cap), nl = std::min(L.left.size(), left_cap);
  if (nf) memcpy(faulty_pos, L.pos.data(), nf * 8), memcpy(faulty_val, L.val.data(), nf * 8);
  if (nl) memcpy(left_rows, L.left.data(), nl * 8);
  *n_faulty = L.n_faulty;
  *n_left = L.n_left;
}

size_t size_engine_chunk(int lanes) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ENG_CHUNK;
  const size_t fit = free_b / 2 / ((size_t)std::max(lanes, 1) * eng_bytes_per_round());
  return std::max(ENG_CHUNK_MIN, std::min(ENG_CHUNK, fit));
}

}  // namespace

extern "C" {

int dgpu_abi_version(void) { return DGPU_ABI_VERSION; }
const char* dgpu_last_error(void) { return g_last_error.c_str(); }

int dgpu_scheme_from_name(const char* name) {
  if (!name) return set_err(DGPU_EINVAL, "null scheme name");
  if (name[0] == 0 || !strcmp(name, "pedersen-bls-chained")) return DGPU_SCHEME_CHAINED;
  if (!strcmp(name, "pedersen-bls-unchained")) return DGPU_SCHEME_UNCHAINED;
  if (!strcmp(name, "bls-unchained-on-g1")) return DGPU_SCHEME_UNCHAINED_G1;
  if (!strcmp(name, "bls-unchained-g1-rfc9380")) return DGPU_SCHEME_G1_RFC9380;
  return set_err(DGPU_EINVAL, "scheme [%s] is not valid", name);
}

void dgpu_shard_range(size_t n, int ndev, int k, size_t* lo, size_t* hi) {
  // contiguous shards of a multiple of 8 items (whole verdict-bitmap bytes),
  // the last one takes the remainder
  if (ndev < 1) ndev = 1;
  size_t per = (n + (size_t)ndev - 1) / (size_t)ndev;
  per = (per + 7) & ~(size_t)7;
  size_t a = std::min(n, (size_t)k * per), b = std::min(n, a + per);
  if (k < 0) a = b = 0;
  if (lo) *lo = a;
  if (hi) *hi = b;
}

int dgpu_open(int device, dgpu_ctx** out) {
  if (!out) return set_err(DGPU_EINVAL, "null out");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return set_err(DGPU_EDEVICE, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= count) return set_err(DGPU_EINVAL, "device %d out of range (%d devices)", device, count);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(DGPU_EDEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  dgpu_ctx* c = new dgpu_ctx();
  c->device = device;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // Shipped thresholds and the documented kernel-family switches
  // (include/drand_gpu.h dgpu_open); nothing else is read from the
  // environment by the shipped library.
  const char* fgv = getenv("DGPU_FE_GS_MAX");
  if (fgv && atol(fgv) >= 0) c->fe_gs_max = (size_t)atol(fgv);
  const char* cev = getenv("DGPU_COF_ENGINE_MAX");
  if (cev && atol(cev) >= 0) c->cof_engine_max = (size_t)atol(cev);
  const char* lv = getenv("DGPU_LANES");
  if (lv && !strcmp(lv, "1")) c->lanes = 1;
  const char* ec = getenv("DGPU_ENG_CHUNK");
  c->eng_chunk = (ec && atol(ec) >= 4096) ? (size_t)atol(ec) : size_engine_chunk(c->lanes);
  const char* kcv = getenv("DGPU_KB_CHAIN");
  if (kcv && !strcmp(kcv, "lanes")) c->kb_thread = false;
  const char* lnv = getenv("DGPU_LINES");
  if (lnv && !strcmp(lnv, "engine")) c->lines_thread = false;
  const char* mlv = getenv("DGPU_MILLER");
  if (mlv && !strcmp(mlv, "lanes12")) c->miller6 = false;
  const char* fsv = getenv("DGPU_FESEG");
  if (fsv && !strcmp(fsv, "lanes12")) c->feseg6 = false;
  const char* tmv = getenv("DGPU_THR_MIN");
  if (tmv && atol(tmv) >= 0) c->thr_min = (size_t)atol(tmv);
  const char* rmv = getenv("DGPU_RLC_MIN");
  if (rmv && atol(rmv) >= 0) c->rlc_min = (size_t)atol(rmv);
  const char* fev = getenv("DGPU_FE");
  if (fev && !strcmp(fev, "gs")) c->fe_gs = true;
#ifdef DG_AB_KNOBS
  // Variants measured and not shipped, tuning knobs and test hooks: read only
  // by the A/B build (drand_amd/libdrand_gpu_ab.so, __graft_entry__.build;
  // tools/build_variant.sh), never by the shipped library.
  const char* dov = getenv("DGPU_DEC_OVERLAP");
  if (dov && !strcmp(dov, "0")) c->dec_overlap = false;
  const char* msv = getenv("DGPU_MSM_SEG");
  if (msv && !strcmp(msv, "0")) c->msm_seg = false;
  const char* lsv = getenv("DGPU_LANE_SLICES");
  if (lsv && atol(lsv) >= 2 && atol(lsv) <= 64) c->lane_slices = (size_t)atol(lsv);
  const char* knv = getenv("DGPU_KB_NORM");
  if (knv) c->kb_norm_chain = strcmp(knv, "planes") != 0;
  const char* rds = getenv("DGPU_RLC_DESCENT_STEP");
  if (rds && atoi(rds) >= 1 && atoi(rds) <= 8) c->rlc_descent_step = atoi(rds);
  const char* rlv = getenv("DGPU_RLC_LOCALIZE");
  if (rlv && !strcmp(rlv, "0")) c->rlc_localize = false;
  const char* gl = getenv("DGPU_G1_LINES");
  if (gl && !strcmp(gl, "buffer")) c->fused_fixed = false;
  const char* sgv = getenv("DGPU_SUBGROUP");
  if (sgv && !strcmp(sgv, "decode")) c->decode_subgroup = true;
  const char* rcv = getenv("DGPU_RECOVER");
  if (rcv && !strcmp(rcv, "exact")) c->recover_exact = true;
  const char* rrv = getenv("DGPU_RECOVER_ROWS");
  if (rrv && !strcmp(rrv, "0")) c->recover_rows = false;
  const char* rwb = getenv("DGPU_RECOVER_WIDE_BUDGET");
  if (rwb && atol(rwb) >= 1) c->recw_budget = (size_t)atol(rwb);
  const char* kic = getenv("DGPU_KB_INV_CHAIN");
  if (kic && atol(kic) >= 1) c->kb_inv_chain = (size_t)atol(kic);
  const char* ktf = getenv("DGPU_KB_TEST_FLAG");
  if (ktf && atol(ktf) >= 1) c->kb_test_flag = (size_t)atol(ktf);
  const char* mmv = getenv("DGPU_TEST_MILLER_MARK");
  if (mmv) c->test_miller_mark = !strcmp(mmv, "1");
  const char* fmv = getenv("DGPU_TEST_FE_MARK");
  if (fmv) c->test_fe_mark = !strcmp(fmv, "1");
  const char* kpv = getenv("DGPU_KB_PAIR");
  if (kpv) c->kb_pair = !strcmp(kpv, "1");
  const char* rnv = getenv("DGPU_REDUCE_NORM");
  if (rnv) c->reduce_norm = !strcmp(rnv, "1");
  const char* lwv = getenv("DGPU_LINES_WAVE");
  if (lwv) c->lines_wave = !strcmp(lwv, "1");
  const char* xwv = getenv("DGPU_ENG_XW");
  if (xwv) c->eng_xw = atoi(xwv) & 3;
  const char* stv = getenv("DGPU_STAGE");
  if (stv && !strcmp(stv, "pageable")) c->stage_pageable = true;
  const char* krv = getenv("DGPU_KEYED_RANGE");
  if (krv && atol(krv) >= 1) c->keyed_range = (size_t)atol(krv);
  const char* tso = getenv("DGPU_TEST_STAGE_ONLY");
  if (tso && !strcmp(tso, "1")) c->test_stage_only = true;
  const char* tac = getenv("DGPU_TEST_ALLOC_CAP");
  // process-global: written at every dgpu_open of this build, so a context opened without the knob resets it
  g_test_alloc_cap = tac && atol(tac) >= 0 ? (size_t)atol(tac) : 0;
  {  // the fast group-law paths' generic redo on every item (kernels.cuh DG_FORCE_EXC); written at every
     // dgpu_open of this build, so a context opened without the knob resets it
    const char* fev2 = getenv("DGPU_TEST_FORCE_EXC");
    const int force = fev2 && !strcmp(fev2, "1") ? 1 : 0;
    const hipError_t fe = hipMemcpyToSymbol(HIP_SYMBOL(g_dg_force_exc), &force, sizeof(force));
    if (fe != hipSuccess) {
      delete c;
      return set_err(DGPU_EDEVICE, "DGPU_TEST_FORCE_EXC: %s", hipGetErrorString(fe));
    }
  }
#endif
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->lane_ev[0], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->lane_ev[1], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->cof_ev[0], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->cof_ev[1], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    dgpu_close(c);
    return set_err(DGPU_EDEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  if (upload_eng_consts(&c->eng_consts, nullptr) != DGPU_OK) {
    std::string msg = g_last_error;
    dgpu_close(c);
    return set_err(DGPU_EDEVICE, "%s", msg.c_str());
  }
  g_last_error.clear();  // a new context starts without an earlier context's message on this thread
  *out = c;
  return DGPU_OK;
}

void dgpu_close(dgpu_ctx* c) {
  if (!c) return;
  // teardown: nothing to do about a failure here, the results are dropped on purpose
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  if (c->done) (void)hipEventSynchronize(c->done);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->lane_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->cof_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->done) (void)hipEventDestroy(c->done);
  if (c->ky_ev) (void)hipEventDestroy(c->ky_ev);
  if (c->ky_host) (void)hipHostFree(c->ky_host);
  if (c->stream_copy) {
    (void)hipStreamSynchronize(c->stream_copy);
    (void)hipStreamDestroy(c->stream_copy);
  }
  for (int k = 0; k < 2; ++k) {
    if (c->ring_ev[k]) (void)hipEventDestroy(c->ring_ev[k]);
    if (c->ring[k]) (void)hipHostFree(c->ring[k]);
  }
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // the device buffers go with the context: every stream that used them has been drained
}

int dgpu_set_pubkey(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t len) {
  if (!c || !pk) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, len, &k);
  if (rc) return rc;
  c->cur = k;
  return DGPU_OK;
}

int dgpu_verify_batch_device(dgpu_ctx* c, int scheme, size_t n, const uint64_t* d_rounds, const uint8_t* d_sigs,
                             size_t sig_stride, const uint32_t* d_sig_len, const uint8_t* d_prev, size_t prev_stride,
                             const uint32_t* d_prev_len, int mode, uint64_t rlc_seed, uint8_t* d_bits,
                             uint8_t* d_reason, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  const verify_args a{scheme, n, beacon_src(d_rounds, d_prev, prev_stride, d_prev_len, scheme == DGPU_SCHEME_CHAINED),
                      d_sigs, sig_stride, d_sig_len, mode, rlc_seed};
  return verify_device_locked(c, c->cur, a, d_bits, d_reason, s);
}

int dgpu_verify_batch(dgpu_ctx* c, int scheme, size_t n, const uint64_t* rounds, const uint8_t* sigs,
                      size_t sig_stride, const uint32_t* sig_len, const uint8_t* prev, size_t prev_stride,
                      const uint32_t* prev_len, int mode, uint64_t rlc_seed, uint8_t* verdict_bits, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const verify_args a{scheme, n, beacon_src(rounds, prev, prev_stride, prev_len, scheme == DGPU_SCHEME_CHAINED), sigs,
                      sig_stride, sig_len, mode, rlc_seed};
  return verify_host_locked(c, c->cur, a, verdict_bits, reason);
}

int dgpu_verify_beacons(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint64_t* rounds,
                        const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len, const uint8_t* prev,
                        size_t prev_stride, const uint32_t* prev_len, int mode, uint64_t rlc_seed,
                        uint8_t* verdict_bits, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, pk_len, &k);
  if (rc) return rc;
  const verify_args a{scheme, n, beacon_src(rounds, prev, prev_stride, prev_len, scheme == DGPU_SCHEME_CHAINED), sigs,
                      sig_stride, sig_len, mode, rlc_seed};
  return verify_host_locked(c, k, a, verdict_bits, reason);
}

int dgpu_verify_beacons_device(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n,
                               const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride,
                               const uint32_t* d_sig_len, const uint8_t* d_prev, size_t prev_stride,
                               const uint32_t* d_prev_len, int mode, uint64_t rlc_seed, uint8_t* d_bits,
                               uint8_t* d_reason, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, pk_len, &k);
  if (rc) return rc;
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  const verify_args a{scheme, n, beacon_src(d_rounds, d_prev, prev_stride, d_prev_len, scheme == DGPU_SCHEME_CHAINED),
                      d_sigs, sig_stride, d_sig_len, mode, rlc_seed};
  return verify_device_locked(c, k, a, d_bits, d_reason, s);
}

int dgpu_decode_rows_device(dgpu_ctx* c, size_t n, const uint8_t* d_rows, size_t rows_bytes, const uint64_t* d_row_off,
                            const uint32_t* d_row_len, uint64_t* d_rounds, uint8_t* d_sigs, size_t sig_stride,
                            uint32_t* d_sig_len, uint8_t* d_prev, size_t prev_stride, uint32_t* d_prev_len, uint8_t* d_ok,
                            void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (n == 0) return DGPU_OK;
  if (!d_row_off || !d_row_len || !d_rounds || !d_sigs || !d_sig_len || !d_prev_len || !d_ok ||
      (!d_rows && rows_bytes) || (!d_prev && prev_stride))
    return set_err(DGPU_EINVAL, "null row or record buffer");
  if (n > (size_t)0x7fffffff * INGEST_ROWS_PER_WAVE) return set_err(DGPU_EINVAL, "too many rows");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  return launch_n(k_ingest_rows, n, INGEST_ROWS_PER_WAVE, s, n, d_rows, rows_bytes, d_row_off, d_row_len, d_rounds, d_sigs,
                  sig_stride, d_sig_len, d_prev, prev_stride, d_prev_len, d_ok);
}

int dgpu_verify_rows(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint8_t* base,
                     const uint64_t* row_off, const uint32_t* row_len, size_t sig_stride, size_t prev_stride, int mode,
                     uint64_t rlc_seed, uint64_t* rounds_out, uint8_t* row_ok, uint8_t* verdict_bits, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, pk_len, &k);
  if (rc) return rc;
  // (the record pointers are the context's buffers once the call is staged)
  rows_src R = rows_src_of(base, row_off, row_len, nullptr, sig_stride, prev_stride);
  const verify_args a{scheme, n, rows_records_src(&R, prev_stride, scheme == DGPU_SCHEME_CHAINED),
                      nullptr, sig_stride, nullptr, mode, rlc_seed};
  return verify_rows_locked(c, k, a, rounds_out, row_ok, verdict_bits, reason);
}

int dgpu_faulty_rounds_device(dgpu_ctx* c, uint64_t first, size_t count, size_t n, const uint64_t* d_keys,
                              const uint8_t* d_row_ok, const uint64_t* d_rounds, const uint8_t* d_reason,
                              uint64_t* d_faulty_pos, uint64_t* d_faulty_val, size_t faulty_cap, uint64_t* d_left_rows,
                              size_t left_cap, uint64_t* d_counts, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (count == 0) return DGPU_OK;
  int rc = check_range_args(first, count, n);
  if (rc) return rc;
  if (!d_counts || (n && (!d_keys || !d_row_ok || !d_rounds || !d_reason)) ||
      (faulty_cap && (!d_faulty_pos || !d_faulty_val)) || (left_cap && !d_left_rows))
    return set_err(DGPU_EINVAL, "null row, list or count buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  return faulty_rounds_locked(c, first, count, n, d_keys, d_row_ok, d_rounds, d_reason, d_faulty_pos, d_faulty_val,
                              faulty_cap, d_left_rows, left_cap, d_counts, s);
}

int dgpu_check_rows(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint8_t* base,
                    const uint64_t* row_off, const uint32_t* row_len, const uint64_t* keys, size_t sig_stride,
                    size_t prev_stride, int mode, uint64_t rlc_seed, uint64_t first, size_t count,
                    uint64_t* faulty_pos, uint64_t* faulty_val, size_t faulty_cap, uint64_t* n_faulty,
                    uint64_t* left_rows, size_t left_cap, uint64_t* n_left, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = check_rows_args(n, base, row_off, row_len, keys, first, count, faulty_pos, faulty_val, faulty_cap, n_faulty,
                           left_rows, left_cap, n_left);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  if ((rc = get_key_locked(c, scheme, pk, pk_len, &k))) return rc;
  rows_src R = rows_src_of(base, row_off, row_len, keys, sig_stride, prev_stride);
  const verify_args a{scheme, n, rows_records_src(&R, prev_stride, scheme == DGPU_SCHEME_CHAINED),
                      nullptr, sig_stride, nullptr, mode, rlc_seed};
  check_lists L;
  if ((rc = check_rows_locked(c, k, a, first, count, faulty_cap, left_cap, L, reason))) return rc;
  check_lists_store(L, faulty_pos, faulty_val, faulty_cap, n_faulty, left_rows, left_cap, n_left);
  return DGPU_OK;
}

// The arguments of the two segment entry points that no other call has.
static int check_segment_args(int scheme, uint64_t first_round, size_t n, const uint8_t* seed_prev,
                              size_t seed_prev_len) {
  if (seed_prev_len > sizeof(msg_src_linked::seed))
    return set_err(DGPU_EINVAL, "seed_prev_len %zu > %zu", seed_prev_len, sizeof(msg_src_linked::seed));
  if (n && first_round + (uint64_t)(n - 1) < first_round)
    return set_err(DGPU_EINVAL, "rounds %llu + %zu overflow", (unsigned long long)first_round, n);
  if (scheme == DGPU_SCHEME_CHAINED && seed_prev_len && !seed_prev) return set_err(DGPU_EINVAL, "null seed_prev");
  return DGPU_OK;
}

int dgpu_verify_segment(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_round, size_t n,
                        const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len, const uint8_t* seed_prev,
                        size_t seed_prev_len, int mode, uint64_t rlc_seed, uint8_t* verdict_bits, uint8_t* reason,
                        uint8_t* randomness32) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = check_segment_args(scheme, first_round, n, seed_prev, seed_prev_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  if ((rc = get_key_locked(c, scheme, pk, pk_len, &k))) return rc;
  const verify_args a{scheme, n,
                      linked_src(first_round, sigs, sig_stride, sig_len, seed_prev, seed_prev_len,
                                 scheme == DGPU_SCHEME_CHAINED),
                      sigs, sig_stride, sig_len, mode, rlc_seed};
  return verify_host_locked(c, k, a, verdict_bits, reason, randomness32);
}

int dgpu_verify_segment_device(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_round,
                               size_t n, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_len,
                               const uint8_t* seed_prev, size_t seed_prev_len, int mode, uint64_t rlc_seed,
                               uint8_t* d_bits, uint8_t* d_reason, uint8_t* d_randomness32, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = check_segment_args(scheme, first_round, n, seed_prev, seed_prev_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  if ((rc = get_key_locked(c, scheme, pk, pk_len, &k))) return rc;
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  // the seed travels inside the source (a kernel argument): seed_prev is not read after this line
  const verify_args a{scheme, n,
                      linked_src(first_round, d_sigs, sig_stride, d_sig_len, seed_prev, seed_prev_len,
                                 scheme == DGPU_SCHEME_CHAINED),
                      d_sigs, sig_stride, d_sig_len, mode, rlc_seed};
  return verify_device_locked(c, k, a, d_bits, d_reason, s, d_randomness32);
}

// The arguments of the halo form (a shard of a linked segment).
static int check_shard_args(int scheme, uint64_t first_round, size_t n, const uint8_t* d_halo,
                            const uint32_t* d_halo_len) {
  if (n && first_round + (uint64_t)(n - 1) < first_round)
    return set_err(DGPU_EINVAL, "rounds %llu + %zu overflow", (unsigned long long)first_round, n);
  if (scheme == DGPU_SCHEME_CHAINED && n && (!d_halo || !d_halo_len))
    return set_err(DGPU_EINVAL, "a chained shard needs its halo (d_halo, d_halo_len)");
  return DGPU_OK;
}

int dgpu_verify_segment_shard_device(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_round,
                                     size_t n, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_len,
                                     const uint8_t* d_halo, const uint32_t* d_halo_len, int mode, uint64_t rlc_seed,
                                     uint8_t* d_bits, uint8_t* d_reason, uint8_t* d_randomness32, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = check_shard_args(scheme, first_round, n, d_halo, d_halo_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  if ((rc = get_key_locked(c, scheme, pk, pk_len, &k))) return rc;
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  // the halo is read by the kernels, in stream order: the host never looks at it
  const verify_args a{scheme, n,
                      halo_src(first_round, d_sigs, sig_stride, d_sig_len, d_halo, d_halo_len,
                               scheme == DGPU_SCHEME_CHAINED),
                      d_sigs, sig_stride, d_sig_len, mode, rlc_seed};
  return verify_device_locked(c, k, a, d_bits, d_reason, s, d_randomness32);
}

int dgpu_rlc_root_bytes(int scheme) {
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  return 2 * rlc_geom_of(sig_on_g1(scheme)).jw * 4;
}

// Step 1 of the per-rank RLC protocol for the device-resident shard `a`
// (any message source): its root to d_root, the shard kept pending on the
// context for dgpu_rlc_finish_device.
static int rlc_root_pending_locked(dgpu_ctx* c, const verify_args& a, const uint8_t* pk, size_t pk_len,
                                   uint8_t* d_root, void* stream) {
  const int scheme = a.scheme;
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, pk_len, &k);
  if (rc) return rc;
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  if ((rc = check_args(c, k, a))) return rc;
  c->rlc_pending = false;
  if ((rc = rlc_shard_root_locked(c, a, d_root, s))) return rc;
  c->rlc_args = a;
  memcpy(c->rlc_pk, pk, pk_len);
  c->rlc_pk_len = pk_len;
  c->rlc_pending = true;
  return DGPU_OK;
}

int dgpu_rlc_root_device(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n,
                         const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_len,
                         const uint8_t* d_prev, size_t prev_stride, const uint32_t* d_prev_len, uint64_t rlc_seed,
                         uint8_t* d_root, void* stream) {
  if (!c || !d_root) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  const verify_args a{scheme, n, beacon_src(d_rounds, d_prev, prev_stride, d_prev_len, scheme == DGPU_SCHEME_CHAINED),
                      d_sigs, sig_stride, d_sig_len, DGPU_MODE_RLC, rlc_seed};
  return rlc_root_pending_locked(c, a, pk, pk_len, d_root, stream);
}

int dgpu_rlc_root_segment_device(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_round,
                                 size_t n, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_len,
                                 const uint8_t* seed_prev, size_t seed_prev_len, const uint8_t* d_halo,
                                 const uint32_t* d_halo_len, uint64_t rlc_seed, uint8_t* d_root, void* stream) {
  if (!c || !d_root) return set_err(DGPU_EINVAL, "null argument");
  const bool chained = scheme == DGPU_SCHEME_CHAINED;
  int rc = d_halo ? check_shard_args(scheme, first_round, n, d_halo, d_halo_len)
                  : check_segment_args(scheme, first_round, n, seed_prev, seed_prev_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  // (the seed form carries the seed by value, the halo form the two device
  // pointers: the pending source keeps either until the finish step)
  const verify_args a{scheme, n,
                      d_halo ? halo_src(first_round, d_sigs, sig_stride, d_sig_len, d_halo, d_halo_len, chained)
                             : linked_src(first_round, d_sigs, sig_stride, d_sig_len, seed_prev, seed_prev_len, chained),
                      d_sigs, sig_stride, d_sig_len, DGPU_MODE_RLC, rlc_seed};
  return rlc_root_pending_locked(c, a, pk, pk_len, d_root, stream);
}

int dgpu_rlc_finish_device(dgpu_ctx* c, size_t n_roots, const uint8_t* d_roots, uint8_t* d_bits, uint8_t* d_reason,
                           void* stream) {
  if (!c || !d_roots || n_roots == 0) return set_err(DGPU_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  if (!c->rlc_pending) return set_err(DGPU_EINVAL, "no pending dgpu_rlc_root_device on this context");
  c->rlc_pending = false;
  const verify_args a = c->rlc_args;
  if (a.n && !d_bits) return set_err(DGPU_EINVAL, "null verdict buffer");
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, a.scheme, c->rlc_pk, c->rlc_pk_len, &k);
  if (rc) return rc;
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  bool fail = false;
  if ((rc = rlc_node_check_locked(c, k, n_roots, d_roots, s, &fail)) || a.n == 0) return rc;
  if ((rc = rlc_shard_finish_locked(c, k, a, fail, n_roots, s))) return rc;
  return results_out_locked(c, a, d_bits, nullptr, d_reason, hipMemcpyDeviceToDevice, nullptr, s);
}

int dgpu_verify_recovered(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint8_t* msgs,
                          size_t msg_stride, const uint32_t* msg_len, const uint8_t* sigs, size_t sig_stride,
                          const uint32_t* sig_len, int mode, uint64_t rlc_seed, uint8_t* verdict_bits,
                          uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (n && (!msg_len || (!msgs && msg_stride))) return set_err(DGPU_EINVAL, "null message buffers");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  key_entry* k = nullptr;
  int rc = get_key_locked(c, scheme, pk, pk_len, &k);
  if (rc) return rc;
  static const uint8_t empty = 0;
  const verify_args a{scheme, n, raw_src(msgs ? msgs : &empty, msg_stride, msg_len), sigs, sig_stride, sig_len, mode,
                      rlc_seed};
  return verify_host_locked(c, k, a, verdict_bits, reason);
}

int dgpu_synchronize(dgpu_ctx* c) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->done));
  return DGPU_OK;
}

int dgpu_staging_stats(dgpu_ctx* c, double* device_ms, double* host_ms, uint64_t* bytes) {
  if (!c || !device_ms || !host_ms || !bytes) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  *device_ms = c->last_stage_ms;
  *host_ms = c->last_stage_host_ms;
  *bytes = c->last_stage_bytes;
  return DGPU_OK;
}

int dgpu_set_profiling(dgpu_ctx* c, int enable) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->profile = enable != 0;
  c->n_ev = 0;
  c->ev_overflow = false;
  return DGPU_OK;
}

int dgpu_stage_times(dgpu_ctx* c, float* ms_out, int max_stages, const char** names_out) {
  if (!c || !ms_out) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->ev_overflow)
    return set_err(DGPU_EINVAL, "stage timing: the last call recorded more than %d stage events", STAGE_EVENTS_MAX);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<const char*> names;
  std::vector<float> sums;
  for (int i = 0; i + 1 < c->n_ev; ++i) {
    if (!c->stage_name[i]) continue;
    HIP_TRY(hipEventSynchronize(c->ev[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
    size_t k = 0;
    while (k < names.size() && strcmp(names[k], c->stage_name[i]) != 0) ++k;
    if (k == names.size()) {
      names.push_back(c->stage_name[i]);
      sums.push_back(0.f);
    }
    sums[k] += ms;
  }
  const int n = (int)std::min<size_t>(names.size(), (size_t)std::max(max_stages, 0));
  for (int i = 0; i < n; ++i) {
    ms_out[i] = sums[i];
    if (names_out) names_out[i] = names[i];
  }
  return (int)names.size();  // the count needed (like snprintf): > max_stages means truncated
}

int dgpu_digest_batch(dgpu_ctx* c, int scheme, size_t n, const uint64_t* rounds, const uint8_t* prev,
                      size_t prev_stride, const uint32_t* prev_len, uint8_t* out32) {
  if (!c || !rounds || !out32) return set_err(DGPU_EINVAL, "null argument");
  if (n == 0) return DGPU_OK;
  bool chained = scheme == DGPU_SCHEME_CHAINED;
  if (chained && (!prev_len || (!prev && prev_stride))) return set_err(DGPU_EINVAL, "chained scheme needs previous signatures");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  if ((rc = c->in_rounds.ensure(n * 8))) return rc;
  if ((rc = c->misc.ensure(n * 32))) return rc;
  HIP_TRY(hipMemcpyAsync(c->in_rounds.p, rounds, n * 8, hipMemcpyHostToDevice, s));
  const uint8_t* d_prev = nullptr;
  const uint32_t* d_prev_len = nullptr;
  if (chained) {
    if ((rc = c->in_prev.ensure(n * prev_stride + 1))) return rc;
    if ((rc = c->in_prev_len.ensure(n * 4))) return rc;
    if ((rc = lengths_check(prev_len, n, prev_stride, PREV_LEN_FMT))) return rc;
    if (prev_stride) HIP_TRY(hipMemcpyAsync(c->in_prev.p, prev, n * prev_stride, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->in_prev_len.p, prev_len, n * 4, hipMemcpyHostToDevice, s));
    d_prev = c->in_prev.u8();
    d_prev_len = c->in_prev_len.u32();
  }
  RC_TRY(launch_n(k_digest, n, 256, s, n, c->in_rounds.u64(), d_prev, prev_stride, d_prev_len, chained ? 1 : 0,
                  c->misc.u8()));
  HIP_TRY(hipMemcpyAsync(out32, c->misc.p, n * 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_hash_to_curve(dgpu_ctx* c, int scheme, size_t n, const uint8_t* msgs, size_t msg_stride,
                       const uint32_t* msg_len, uint8_t* out) {
  if (!c || !msg_len || !out || (!msgs && msg_stride)) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  if (n == 0) return DGPU_OK;
  if (int rc = lengths_check(msg_len, n, msg_stride, MSG_LEN_FMT)) return rc;
  const bool g1 = sig_on_g1(scheme);
  const size_t ob = g1 ? 48 : 96;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  if ((rc = c->in_msgs.ensure(n * msg_stride + 1)) || (rc = c->in_msg_len.ensure(n * 4)) ||
      (rc = c->misc.ensure(n * ob)))
    return rc;
  if (msg_stride) HIP_TRY(hipMemcpyAsync(c->in_msgs.p, msgs, n * msg_stride, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->in_msg_len.p, msg_len, n * 4, hipMemcpyHostToDevice, s));
  const msg_src m = raw_src(c->in_msgs.u8(), msg_stride, c->in_msg_len.u32());
  if (g1)
    RC_TRY(launch_n(k_hash_to_g1_msgs, n, 256, s, n, m, scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, c->misc.u8()));
  else
    RC_TRY(launch_n(k_hash_to_g2_msgs, n, 256, s, n, m, c->misc.u8()));
  HIP_TRY(hipMemcpyAsync(out, c->misc.p, n * ob, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_hash_to_g2(dgpu_ctx* c, size_t n, const uint8_t* msg32, uint8_t* out96) {
  if (!c || !msg32 || !out96) return set_err(DGPU_EINVAL, "null argument");
  std::vector<uint32_t> len(n, 32);
  return dgpu_hash_to_curve(c, DGPU_SCHEME_CHAINED, n, msg32, 32, len.data(), out96);
}

int dgpu_hash_to_g1(dgpu_ctx* c, int scheme, size_t n, const uint8_t* msg32, uint8_t* out48) {
  if (!c || !msg32 || !out48) return set_err(DGPU_EINVAL, "null argument");
  if (!sig_on_g1(scheme)) return set_err(DGPU_EINVAL, "scheme %d does not sign on G1", scheme);
  std::vector<uint32_t> len(n, 32);
  return dgpu_hash_to_curve(c, scheme, n, msg32, 32, len.data(), out48);
}

}  // extern "C"

static scalar256 scalar_from_be32(const uint8_t* b) {
  scalar256 k;
  for (int w = 0; w < 8; ++w)
    k.w[w] = ((uint32_t)b[31 - 4 * w - 3] << 24) | ((uint32_t)b[31 - 4 * w - 2] << 16) |
             ((uint32_t)b[31 - 4 * w - 1] << 8) | b[31 - 4 * w];
  return k;
}

extern "C" {

int dgpu_sign(dgpu_ctx* c, int scheme, const uint8_t* sk_be32, size_t n, const uint8_t* msgs, size_t msg_stride,
              const uint32_t* msg_len, uint8_t* out_sigs) {
  if (!c || !sk_be32 || !msg_len || !out_sigs || (!msgs && msg_stride)) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  if (n == 0) return DGPU_OK;
  if (int rc = lengths_check(msg_len, n, msg_stride, MSG_LEN_FMT)) return rc;
  const bool g1 = sig_on_g1(scheme);
  const size_t ob = g1 ? 48 : 96;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  if ((rc = c->in_msgs.ensure(n * msg_stride + 1)) || (rc = c->in_msg_len.ensure(n * 4)) ||
      (rc = c->misc.ensure(n * ob)))
    return rc;
  if (msg_stride) HIP_TRY(hipMemcpyAsync(c->in_msgs.p, msgs, n * msg_stride, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->in_msg_len.p, msg_len, n * 4, hipMemcpyHostToDevice, s));
  const msg_src m = raw_src(c->in_msgs.u8(), msg_stride, c->in_msg_len.u32());
  RC_TRY(launch_n(k_sign_msgs, n, 64, s, n, m, g1 ? 1 : 0, scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0,
                  scalar_from_be32(sk_be32), c->misc.u8(), ob));
  HIP_TRY(hipMemcpyAsync(out_sigs, c->misc.p, n * ob, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_decode_g1_points(dgpu_ctx* c, size_t n, const uint8_t* in48, int* rc_out, uint8_t* xy96) {
  if (!c || !in48 || !rc_out) return set_err(DGPU_EINVAL, "null argument");
  if (n == 0) return DGPU_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  g1_points_misc M;
  if ((rc = c->in_msgs.ensure(n * 48)) || (rc = carve(c->misc, &M, n))) return rc;
  HIP_TRY(hipMemcpyAsync(c->in_msgs.p, in48, n * 48, hipMemcpyHostToDevice, s));
  int* const d_rc = M.rc;
  uint8_t* const d_xy = M.xy;
  RC_TRY(launch_n(k_decode_g1_points, n, 64, s, n, c->in_msgs.u8(), d_rc, d_xy));
  HIP_TRY(hipMemcpyAsync(rc_out, d_rc, n * 4, hipMemcpyDeviceToHost, s));
  if (xy96) HIP_TRY(hipMemcpyAsync(xy96, d_xy, n * 96, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_decode_signatures(dgpu_ctx* c, int scheme, size_t n, const uint8_t* sigs, size_t sig_stride,
                           const uint32_t* sig_len, uint8_t* reason, uint8_t* xy) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  if (n == 0) return DGPU_OK;
  if (!sig_len || !reason || (!sigs && sig_stride)) return set_err(DGPU_EINVAL, "null argument");
  const bool g1 = sig_on_g1(scheme);
  const size_t want = g1 ? 48 : 96;
  for (size_t i = 0; i < n; ++i)
    if (sig_len[i] == want && sig_stride < want) return set_err(DGPU_EINVAL, "sig_stride %zu < %zu", sig_stride, want);
  const int nfp = g1 ? 2 : 4;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  c->rlc_pending = false;
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  if ((rc = c->in_sigs.ensure(n * sig_stride + 1)) || (rc = c->in_sig_len.ensure(n * 4)) ||
      (rc = c->lane[0].sig_pts.ensure(n * nfp * FP_WORDS * 4)) || (rc = c->status.ensure(n)) ||
      (rc = c->misc.ensure(n * nfp * 48)))
    return rc;
  if (sig_stride) HIP_TRY(hipMemcpyAsync(c->in_sigs.p, sigs, n * sig_stride, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->in_sig_len.p, sig_len, n * 4, hipMemcpyHostToDevice, s));
  const msg_src m = beacon_src(nullptr, nullptr, 0, nullptr, false);  // no message part: never a bad record
  uint32_t* pts = c->lane[0].sig_pts.u32();
  uint8_t* st = c->status.u8();
  RC_TRY(launch_n(g1 ? k_decode_g1_sigs<msg_src> : k_decode_g2_sigs_sub<msg_src>, n, 256, s, n, c->in_sigs.u8(), sig_stride,
                  c->in_sig_len.u32(), m, pts, st));
  HIP_TRY(hipMemcpyAsync(reason, st, n, hipMemcpyDeviceToHost, s));
  if (xy) {
    RC_TRY(launch_n(k_fp_soa_to_be48, n * nfp, 256, s, n, nfp, pts, 0, c->misc.u8()));
    HIP_TRY(hipMemcpyAsync(xy, c->misc.p, n * nfp * 48, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_decode_pubkey(dgpu_ctx* c, int scheme, const uint8_t* pk, size_t len, uint8_t* xy) {
  if (!c || !pk) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  const bool g2key = sig_on_g1(scheme);
  const size_t want = g2key ? 96 : 48;
  if (len != want)
    return set_err(DGPU_EINVAL, "public key must be %zu bytes (compressed %s), got %zu", want, g2key ? "G2" : "G1", len);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  pubkey_misc M;
  if ((rc = carve(c->misc, &M))) return rc;
  uint8_t *const d_in = M.in, *const d_xy = M.xy;
  uint32_t* const d_pt = M.pt;
  int* const d_rc = M.rc;
  HIP_TRY(hipMemcpyAsync(d_in, pk, want, hipMemcpyHostToDevice, s));
  RC_TRY(launch(g2key ? k_decode_g2_pk : k_decode_g1_pk, dim3(1), dim3(64), s, d_in, d_pt, d_rc));
  const int nfp = g2key ? 4 : 2;
  RC_TRY(launch(k_fp_soa_to_be48, dim3(1), dim3(64), s, 1, nfp, d_pt, g2key ? 0 : 1, d_xy));
  int drc = -1;
  uint8_t host[192];
  HIP_TRY(hipMemcpyAsync(&drc, d_rc, sizeof drc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(host, d_xy, (size_t)nfp * 48, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (drc != DEC_OK) return set_err(DGPU_EINVAL, "public key rejected (decode code %d)", drc);
  if (xy) memcpy(xy, host, (size_t)nfp * 48);
  return DGPU_OK;
}

int dgpu_derive_pubkey(dgpu_ctx* c, int scheme, const uint8_t* sk_be32, uint8_t* pk_out, size_t pk_len) {
  if (!c || !sk_be32 || !pk_out) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  const size_t want = sig_on_g1(scheme) ? 96 : 48;
  if (pk_len != want) return set_err(DGPU_EINVAL, "pk_len must be %zu", want);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  stream_order ord(c, c->stream);
  int rc = c->misc.ensure(128);
  if (rc) return rc;
  RC_TRY(launch(sig_on_g1(scheme) ? k_derive_pubkey_g2 : k_derive_pubkey, dim3(1), dim3(64), c->stream,
                scalar_from_be32(sk_be32), c->misc.u8()));
  HIP_TRY(hipMemcpyAsync(pk_out, c->misc.p, want, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DGPU_OK;
}

int dgpu_make_chain(dgpu_ctx* c, int scheme, const uint8_t* sk_be32, size_t n_seg, size_t seg_len,
                    const uint64_t* first_round, const uint8_t* seed_prev, const uint32_t* seed_prev_len,
                    uint8_t* sigs_out) {
  if (!c || !sk_be32 || !first_round || !sigs_out) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  bool chained = scheme == DGPU_SCHEME_CHAINED;
  if (chained && (!seed_prev || !seed_prev_len)) return set_err(DGPU_EINVAL, "chained scheme needs seed_prev");
  if (n_seg == 0 || seg_len == 0) return DGPU_OK;
  scalar256 sk = scalar_from_be32(sk_be32);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  stream_scratch<4> tmp(s);
  DevBuf &d_first = tmp.b[0], &d_prev = tmp.b[1], &d_plen = tmp.b[2], &d_sigs = tmp.b[3];
  if ((rc = d_first.ensure(n_seg * 8)) || (rc = d_prev.ensure(n_seg * 96)) || (rc = d_plen.ensure(n_seg * 4)) ||
      (rc = d_sigs.ensure(n_seg * seg_len * 96)))
    return rc;
  std::vector<uint8_t> pv(n_seg * 96, 0);
  std::vector<uint32_t> pl(n_seg, 0);
  if (chained) {
    for (size_t i = 0; i < n_seg; ++i) {
      pl[i] = seed_prev_len[i] > 96 ? 96 : seed_prev_len[i];
      memcpy(&pv[i * 96], seed_prev + i * 96, pl[i]);
    }
  }
  hipError_t e = hipMemcpyAsync(d_first.p, first_round, n_seg * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_prev.p, pv.data(), n_seg * 96, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_plen.p, pl.data(), n_seg * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_sigs.p, 0, n_seg * seg_len * 96, s);
  if (e != hipSuccess) return set_err(DGPU_EDEVICE, "make_chain: %s", hipGetErrorString(e));
  for (size_t j = 0; j < seg_len; ++j) {
    // segment-major output: round j of segment s at (s*seg_len + j)*96
    uint8_t* const out = d_sigs.u8() + j * 96;
    if (sig_on_g1(scheme))
      RC_TRY(launch_n(k_sign_step_g1, n_seg, 64, s, n_seg, d_first.u64(), j, scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, sk,
                      out, seg_len * 96));
    else
      RC_TRY(launch_n(k_sign_step, n_seg, 64, s, n_seg, d_first.u64(), j, d_prev.u8(), d_plen.u32(), chained ? 1 : 0, sk,
                      out, seg_len * 96));
  }
  e = hipMemcpyAsync(sigs_out, d_sigs.p, n_seg * seg_len * 96, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return set_err(DGPU_EDEVICE, "make_chain: %s", hipGetErrorString(e));
  return DGPU_OK;
}

}  // extern "C"

#include "threshold_host.h"
#include "keyed_host.h"
#include "multi_gpu.h"
