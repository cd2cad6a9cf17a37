// Threshold (t-of-n) host code behind the C ABI: group install
// (dgpu_set_group[_scheme]), recovery (dgpu_recover_batch[_device]; the
// multi-GPU driver in multi_gpu.h shards over recover_device_locked) and the
// partial-signing data tool (dgpu_make_partials[_scheme]).  Included by
// capi.hip (one translation unit: the kernels and the context live there).
//
// A group signs on G2 with G1 commitments (pedersen-bls-*) or on G1 with G2
// commitments (bls-unchained-on-g1, -g1-rfc9380; recover_g1.cuh).  The walk
// is one sequence of stages for both; what differs per group sits in the
// small helpers below (hash, decode, MSM, finish, the batched check's
// other-group combination, the pairing jobs).

namespace {

// Bytes of one recovered signature / of a full partial under the installed group.
size_t group_sig_bytes(const dgpu_ctx* c) { return c->grp_g1 ? 48 : 96; }
size_t group_partial_bytes(const dgpu_ctx* c) { return 2 + group_sig_bytes(c); }

// ---------------------------------------------------------------- group install
// Decode the t compressed commitments (G2: 96 bytes each, else 48-byte G1)
// into dst (affine SoA) and read back the per-commitment decode codes: the
// first rejected one fails the call with DGPU_EINVAL.  Synchronous on the
// context's stream.
int decode_commits_locked(dgpu_ctx* c, bool g2, int t, const uint8_t* commits, DevBuf* dst) {
  const size_t cb = g2 ? 96 : 48;
  hipStream_t s = c->stream;
  int rc;
  commits_misc M;
  if ((rc = carve(c->misc, &M, (size_t)t, cb)) ||
      (rc = dst->ensure((size_t)t * (g2 ? (size_t)G2A_WORDS : 2 * FP_LIMBS) * 4)))
    return rc;
  uint8_t* const d_in = M.in;
  int* const d_rc = M.rc;
  HIP_TRY(hipMemcpyAsync(d_in, commits, (size_t)t * cb, hipMemcpyHostToDevice, s));
  RC_TRY(launch_n(g2 ? k_decode_commits_g2 : k_decode_commits, t, 64, s, t, d_in, dst->u32(), d_rc));
  std::vector<int> hrc(t);
  HIP_TRY(hipMemcpyAsync(hrc.data(), d_rc, t * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int j = 0; j < t; ++j)
    if (hrc[j] != DEC_OK) return set_err(DGPU_EINVAL, "group commitment %d rejected (decode code %d)", j, hrc[j]);
  return DGPU_OK;
}

// A G2-signature group: t compressed G1 commitments, decoded in place -- the
// installed group is cleared first, so a rejected call leaves none.
int set_group_g2_locked(dgpu_ctx* c, int t, int n, const uint8_t* commits48) {
  hipStream_t s = c->stream;
  int rc;
  c->grp_t = 0;
  if ((rc = decode_commits_locked(c, false, t, commits48, &c->grp_commits))) return rc;
  if ((rc = c->grp_table.ensure((size_t)n * 2 * FP_LIMBS * 4)) ||
      (rc = c->grp_wtab.ensure((size_t)n * 8 * REC_WTAB_WORDS * 4)))
    return rc;
  RC_TRY(launch_n(k_pubpoly_table, n, 64, s, n, t, c->grp_commits.u32(), c->grp_table.u32()));
  RC_TRY(launch_n(k_pubpoly_wtable, 8 * (size_t)n, 64, s, n, c->grp_table.u32(), c->grp_wtab.u32()));
  HIP_TRY(hipStreamSynchronize(s));
  c->grp_t = t;
  c->grp_n = n;
  c->grp_scheme = DGPU_SCHEME_CHAINED;
  c->grp_g1 = false;
  return DGPU_OK;
}

// A G1-signature group: t compressed G2 commitments.  Everything is decoded
// and checked in staging buffers first, so a rejected call leaves the
// installed group (of either kind) as it was.
int set_group_g1_locked(dgpu_ctx* c, int scheme, int t, int n, const uint8_t* commits96) {
  hipStream_t s = c->stream;
  int rc;
  if ((rc = decode_commits_locked(c, true, t, commits96, &c->grp_stage))) return rc;
  // VerifyRecovered's key C_0: decoded with its fixed-Q line table as
  // dgpu_set_pubkey does, into the group's own entry (the key cache keeps its 8)
  key_entry fresh;
  if ((rc = decode_g2_key_locked(c, &fresh, commits96))) return rc;
  c->grp_t = 0;
  c->grp_key.consts = std::move(fresh.consts);
  c->grp_key.table = std::move(fresh.table);
  c->grp_key.used = true;
  c->grp_key.g2key = true;
  const size_t cw = (size_t)t * G2A_WORDS * 4;
  if ((rc = c->grp_commits.ensure(cw)) || (rc = c->grp_table.ensure((size_t)n * G2A_WORDS * 4)) ||
      (rc = c->grp_wtab.ensure((size_t)n * 8 * G2A_WORDS * 4)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->grp_commits.p, c->grp_stage.p, cw, hipMemcpyDeviceToDevice, s));
  RC_TRY(launch_n(k_pubpoly_table_g2, n, 64, s, n, t, c->grp_commits.u32(), c->grp_table.u32()));
  RC_TRY(launch_n(k_pubpoly_wtable_g2, 8 * (size_t)n, 64, s, n, c->grp_table.u32(), c->grp_wtab.u32()));
  HIP_TRY(hipStreamSynchronize(s));
  c->grp_t = t;
  c->grp_n = n;
  c->grp_scheme = scheme;
  c->grp_g1 = true;
  return DGPU_OK;
}

// dgpu_set_group_scheme and dgpu_set_group_wide: one body, the threshold limit given.
int set_group_checked(dgpu_ctx* c, int scheme, int t, int n, const uint8_t* commits, size_t commit_len, int max_t) {
  if (!c || !commits) return set_err(DGPU_EINVAL, "null argument");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  const bool g1 = sig_on_g1(scheme);
  const size_t want = g1 ? 96 : 48;
  if (commit_len != want)
    return set_err(DGPU_EINVAL, "commitments of scheme %d are %zu bytes (compressed %s), got %zu", scheme, want,
                   g1 ? "G2" : "G1", commit_len);
  if (t < 1 || t > max_t) return set_err(DGPU_EINVAL, "threshold t=%d outside [1, %d]", t, max_t);
  if (n < t || n > 65536) return set_err(DGPU_EINVAL, "group size n=%d invalid for t=%d", n, t);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  stream_order ord(c, c->stream);
  // the group's tables may still be read by an earlier asynchronous recovery
  HIP_TRY(hipEventSynchronize(c->done));
  return g1 ? set_group_g1_locked(c, scheme, t, n, commits) : set_group_g2_locked(c, t, n, commits);
}

}  // namespace

extern "C" {

int dgpu_set_group_scheme(dgpu_ctx* c, int scheme, int t, int n, const uint8_t* commits, size_t commit_len) {
  return set_group_checked(c, scheme, t, n, commits, commit_len, RECOVER_MAX_T);
}

// (the installed group's t selects the recovery path: above RECOVER_MAX_T the wide one)
int dgpu_set_group_wide(dgpu_ctx* c, int scheme, int t, int n, const uint8_t* commits, size_t commit_len) {
  static_assert(RECOVER_WIDE_MAX_T == DGPU_MAX_THRESHOLD, "one limit");
  return set_group_checked(c, scheme, t, n, commits, commit_len, DGPU_MAX_THRESHOLD);
}

int dgpu_set_group(dgpu_ctx* c, int t, int n, const uint8_t* commits48) {
  return dgpu_set_group_scheme(c, DGPU_SCHEME_CHAINED, t, n, commits48, 48);
}

}  // extern "C"

namespace {

// ---------------------------------------------------------------- recovery
// One recovery batch under the installed group: its sizes and the context's
// scratch as the kernels take it (recover_begin_locked fills it).
struct recover_walk {
  size_t n_rounds, m, items;
  int t;
  bool g1;            // G1 signatures: G2 share keys and commitments (recover_g1.cuh)
  uint32_t* h;        // H(msg) per round
  uint32_t* sg;       // decoded partial signatures, per item
  uint8_t* st;        // ST_* per item
  uint32_t* hidx;     // item -> round (the exact path's VerifyPartial)
  uint32_t* keys;     // share key Eval(i) per item
  uint32_t* idx;      // share index per item
  uint32_t *sel, *xs; // the t selected items of a round, their indices
  uint64_t* dig;      // Lagrange digits (and the batched check's coefficients)
  uint32_t* part;     // the MSM's per-slice sums
  uint32_t* rpts;     // the recovered signature (batched check: B) per round
  uint32_t* rpk;      // the per-round key of the last pairing
  uint8_t* rst;       // ST_* per round
  uint8_t* cls;       // round classes of the batched check
};

// H(msg) of n_rounds 32-byte messages as affine points of the signature group.
int recover_hash_launch(bool g1, int g1dst, size_t n_rounds, const uint8_t* d_msgs, uint32_t* h, hipStream_t s) {
  if (g1) return launch_n(k_hash_to_g1_msgs_pts, n_rounds, 256, s, n_rounds, d_msgs, g1dst, h);
  return launch_n(k_hash_to_g2_msgs_pts, n_rounds, 256, s, n_rounds, d_msgs, h);
}

// Every partial decoded: its signature, share index and share key Eval(i).
int recover_decode_launch(dgpu_ctx* c, const recover_walk& w, const uint8_t* d_parts, size_t stride,
                          const uint32_t* d_plen, hipStream_t s) {
  return launch_n(w.g1 ? k_decode_partials_g1 : k_decode_partials, w.items, 256, s, w.items, d_parts, stride, d_plen,
                  c->grp_n, c->grp_t, c->grp_table.u32(), c->grp_commits.u32(), w.sg, w.keys, w.idx, w.st);
}

// The shared prologue of both recovery paths: the item count validated, the
// scratch ensured, then the hash, the item -> round map (round_of_item: the
// exact path's VerifyPartial reads it) and the partial decode enqueued.
int recover_begin_locked(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs, size_t m, const uint8_t* d_parts,
                         size_t stride, const uint32_t* d_plen, bool round_of_item, hipStream_t s, recover_walk* out) {
  if (!c->grp_t) return set_err(DGPU_ENOKEY, "no threshold group installed (dgpu_set_group)");
  const size_t items = n_rounds * m;
  if (items > 0xFFFFFFFFull) return set_err(DGPU_EINVAL, "batch too large (%zu items)", items);
  const bool g1 = c->grp_g1;
  const size_t key_words = g1 ? (size_t)G2A_WORDS : 2 * FP_LIMBS;
  int rc;
  lane_scratch& L = c->lane[0];
  const bool wide = c->grp_t > RECOVER_MAX_T;  // (recover_wide.cuh: sel, xs and the digits at stride t)
  const size_t t_stride = wide ? (size_t)c->grp_t : (size_t)RECOVER_MAX_T;
  rec_sel_layout sel;
  rec_sel_wide_layout wsel;
  rec_part_layout part;
  static_assert(REC_G1J_WORDS == G1J_WORDS, "one G1 Jacobian SoA");
  if ((rc = c->rec_hidx.ensure(items * 4)) || (rc = c->rec_pk.ensure(items * key_words * 4)) ||
      (rc = c->rec_idx.ensure(items * 4)) || (rc = c->rec_lam.ensure(n_rounds * t_stride * RECOVER_SLOTS * 8)) ||
      (rc = c->rec_pts.ensure(n_rounds * G2A_WORDS * 4)) || (rc = c->rec_vpk.ensure(n_rounds * key_words * 4)) ||
      (rc = c->rec_st.ensure(n_rounds)) || (rc = c->rec_cls.ensure(n_rounds)) ||
      (rc = L.h_pts.ensure(n_rounds * G2A_WORDS * 4)) || (rc = L.sig_pts.ensure(items * G2A_WORDS * 4)) ||
      (rc = c->status.ensure(items)) ||
      (rc = wide ? carve(c->rec_sel, &wsel, n_rounds, t_stride) : carve(c->rec_sel, &sel, n_rounds)) ||
      (rc = carve(c->rec_part, &part, n_rounds, g1 ? G1J_WORDS : G2J_WORDS)))
    return rc;
  recover_walk& w = *out;
  w.n_rounds = n_rounds, w.m = m, w.items = items;
  w.t = c->grp_t;
  w.g1 = g1;
  w.h = L.h_pts.u32();
  w.sg = L.sig_pts.u32();
  w.st = c->status.u8();
  w.hidx = c->rec_hidx.u32();
  w.keys = c->rec_pk.u32();
  w.idx = c->rec_idx.u32();
  w.sel = wide ? wsel.sel : sel.sel;
  w.xs = wide ? wsel.xs : sel.xs;
  w.dig = c->rec_lam.u64();
  w.part = part.slice[0];  // (the kernels take the slices' base)
  w.rpts = c->rec_pts.u32();
  w.rpk = c->rec_vpk.u32();
  w.rst = c->rec_st.u8();
  w.cls = c->rec_cls.u8();
  mark(c, s, "recover_hash");
  RC_TRY(recover_hash_launch(g1, c->grp_scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, n_rounds, d_msgs, w.h, s));
  mark(c, s, "recover_decode");
  if (round_of_item) RC_TRY(launch_n(k_round_of_item, items, 256, s, items, m, w.hidx));
  return recover_decode_launch(c, w, d_parts, stride, d_plen, s);
}

// The G1 recovery MSM's launches (recover_g1.cuh): shared affine window tables
// [1..8] sig_j, then `slices` threads per round of mixed-addition windows.
int recover_msm_g1_locked(dgpu_ctx* c, const recover_walk& w, const uint8_t* d_ok, int slices, hipStream_t s) {
  const size_t ne = w.n_rounds * (size_t)w.t * 8;
  int rc;
  if ((rc = c->rec_tab.ensure(ne * 2 * FP_WORDS * 4)) || (rc = c->rec_tabz.ensure(ne * FP_WORDS * 4)) ||
      (rc = c->rec_tabpre.ensure(ne * FP_WORDS * 4)))
    return rc;
  uint32_t *const tab = c->rec_tab.u32(), *const tabz = c->rec_tabz.u32();
  RC_TRY(launch_n(k_recover_tables_g1, w.n_rounds * (size_t)w.t, 256, s, w.n_rounds, w.t, d_ok, w.sel, w.sg, w.items, tab,
                  tabz));
  RC_TRY(launch_n(k_g1_batch_affine, (ne + 15) / 16, 256, s, ne, tab, tabz, c->rec_tabpre.u32()));
  return launch_n(k_recover_msm_g1, (size_t)slices * w.n_rounds, 256, s, w.n_rounds, w.t, d_ok, w.dig, tab, w.part,
                  slices);
}

// The batched check's G2 MSM (recover.cuh): shared affine window tables
// [1..8] sig_j, then 5 slices of mixed-addition windows.
int recover_msm_g2_locked(dgpu_ctx* c, const recover_walk& w, const uint8_t* d_ok, hipStream_t s) {
  const size_t ne = w.n_rounds * (size_t)w.t * 8;
  int rc;
  if ((rc = c->rec_tab.ensure(ne * G2A_WORDS * 4)) || (rc = c->rec_tabz.ensure(ne * 2 * FP_WORDS * 4)) ||
      (rc = c->rec_tabpre.ensure(ne * FP_WORDS * 4)))
    return rc;
  uint32_t *const tab = c->rec_tab.u32(), *const tabz = c->rec_tabz.u32();
  RC_TRY(launch_n(k_recover_tables, w.n_rounds * (size_t)w.t, 256, s, w.n_rounds, w.t, d_ok, w.sel, w.sg, w.items, tab, tabz));
  RC_TRY(launch_n(k_g2_batch_affine, (ne + 15) / 16, 256, s, ne, tab, tabz, c->rec_tabpre.u32()));
  if (!c->recover_rows)
    return launch_n(k_recover_msm_aff<false>, 5 * w.n_rounds, 256, s, w.n_rounds, w.t, d_ok, w.dig, tab, w.part, 5);
  // the entries as 224-byte rows for the gathers
  if ((rc = c->rec_tab_rows.ensure(ne * G2A_WORDS * 4))) return rc;
  uint32_t* const rows = c->rec_tab_rows.u32();
  RC_TRY(launch_n(k_recover_tab_rows, ne, 256, s, ne, tab, rows));
  return launch_n(k_recover_msm_aff<true>, 5 * w.n_rounds, 256, s, w.n_rounds, w.t, d_ok, w.dig, rows, w.part, 5);
}

// The exact path's G2 MSM: window tables sized to t in private memory (TMAX x
// 8 Jacobian points per thread), four slices per round.
int recover_msm_w4_launch(const recover_walk& w, const uint8_t* d_ok, hipStream_t s) {
  auto msm = w.t <= 8 ? k_recover_msm_w4<8> : w.t <= 16 ? k_recover_msm_w4<16> : w.t <= 24 ? k_recover_msm_w4<24>
                                                                                           : k_recover_msm_w4<32>;
  return launch_n(msm, 4 * w.n_rounds, 256, s, w.n_rounds, w.t, d_ok, w.sel, w.dig, w.sg, w.items, w.part, 4);
}

// ---- a wide group's launches (recover_wide.cuh; t > RECOVER_MAX_T)
bool walk_wide(const recover_walk& w) { return w.t > RECOVER_MAX_T; }

// Candidates / classes before the batched check (exact = false) or the
// selection after the VerifyPartial pairings (exact = true): a block per round.
int recover_walk_wide_launch(dgpu_ctx* c, const recover_walk& w, bool exact, int want_status, uint8_t* d_out,
                             uint8_t* d_ok, hipStream_t s) {
  return launch(exact ? k_recover_walk_wide<true> : k_recover_walk_wide<false>, dim3((unsigned)w.n_rounds), dim3(256), s,
                w.n_rounds, w.m, w.t, want_status, w.idx, w.st, w.sel, w.xs, w.cls, d_ok, d_out, c->grp_commits.u32(),
                w.rpts, w.rpk, w.rst);
}

int recover_lagrange_wide_launch(const recover_walk& w, const uint8_t* d_ok, uint64_t seed, hipStream_t s) {
  return launch(k_recover_lagrange_wide, dim3((unsigned)w.n_rounds), dim3(RECW_LAG_THREADS), s, w.n_rounds, w.t, d_ok,
                w.xs, w.dig, seed);
}

// The MSM of both paths (slices = 5: the batched check's sum too): the batch
// in chunks of rounds whose window tables stay under the budget, enqueued in
// order -- tables, batch inversion, L lanes per (round, slice).
template <class G>
int recover_msm_wide_chunks(dgpu_ctx* c, const recover_walk& w, const uint8_t* d_ok, int slices, int aw, hipStream_t s) {
  const size_t per = recw_chunk_rounds(w.t, w.g1 ? RECW_TERM_BYTES_G1 : RECW_TERM_BYTES_G2, c->recw_budget);
  rec_tab_wide_layout T;
  int rc;
  if ((rc = carve(c->rec_wide_tab, &T, per < w.n_rounds ? per : w.n_rounds, (size_t)w.t, aw, G::JW))) return rc;
  const int L = recw_lanes(w.t);
  for (size_t r0 = 0; r0 < w.n_rounds; r0 += per) {
    const size_t nc = w.n_rounds - r0 < per ? w.n_rounds - r0 : per;
    const size_t ne = nc * (size_t)w.t * 8;
#ifdef DG_AB_KNOBS
    // test hook: under a lowered budget (DGPU_RECOVER_WIDE_BUDGET) a profiled call marks its chunks, so a test
    // can see that the budget took effect (the first four by name; the shipped library marks recover_msm alone)
    static const char* const chunk_mark[4] = {"recover_msm_chunk0", "recover_msm_chunk1", "recover_msm_chunk2",
                                              "recover_msm_chunk3"};
    if (c->recw_budget != RECW_TABLE_BUDGET && r0 / per < 4) mark(c, s, chunk_mark[r0 / per]);
#endif
    RC_TRY(launch_n(k_recover_tables_wide<G>, nc * (size_t)w.t, 256, s, r0, nc, w.t, d_ok, w.sel, w.sg, w.items, T.tab,
                    T.tabz));
    RC_TRY(launch_n(w.g1 ? k_g1_batch_affine : k_g2_batch_affine, (ne + 15) / 16, 256, s, ne, T.tab, T.tabz, T.pre));
    RC_TRY(launch_n(k_recover_msm_wide<G>, nc * (size_t)slices * L, 64, s, w.n_rounds, r0, nc, w.t, L, slices, d_ok, w.dig,
                    T.tab, w.part));
  }
  return DGPU_OK;
}
int recover_msm_wide_locked(dgpu_ctx* c, const recover_walk& w, const uint8_t* d_ok, int slices, hipStream_t s) {
  return w.g1 ? recover_msm_wide_chunks<recw_g1>(c, w, d_ok, slices, 2 * FP_WORDS, s)
              : recover_msm_wide_chunks<recw_g2>(c, w, d_ok, slices, G2A_WORDS, s);
}

// The slices' sums to the round's signature: compressed into d_out's 96-byte
// slot and affine in rpts; slices = 5 (batched check): rpts gets B.
int recover_finish_launch(const recover_walk& w, const uint8_t* d_ok, uint8_t* d_out, int slices, hipStream_t s) {
  return launch_n(w.g1 ? k_recover_finish_g1 : k_recover_finish, w.n_rounds, 64, s, w.n_rounds, d_ok, w.part, d_out, w.rpts,
                  w.rst, slices);
}

// The batched check's combination on the other group: A = the random
// combination of the round's share keys, into rpk (a G2 point per round for
// G1 signatures).
int recover_combine_launch(dgpu_ctx* c, const recover_walk& w, uint8_t* d_ok, hipStream_t s) {
  mark(c, s, w.g1 ? "recover_rlc_g2" : "recover_rlc_g1");
  if (walk_wide(w)) {  // L lanes per round over the key group's window table
    const int L = recw_lanes(w.t);
    return launch_n(w.g1 ? k_recover_rlc_wide<recw_g2> : k_recover_rlc_wide<recw_g1>, w.n_rounds * L, 64, s, w.n_rounds,
                    w.t, L, c->grp_n, w.sel, w.idx, w.dig, c->grp_wtab.u32(), c->grp_commits.u32(), w.cls, d_ok, w.rpk,
                    w.rst);
  }
  return launch_n(w.g1 ? k_recover_rlc_g2 : k_recover_rlc_g1, w.n_rounds, 64, s, w.n_rounds, w.t, c->grp_n, w.sel, w.idx,
                  w.dig, c->grp_wtab.u32(), c->grp_commits.u32(), w.cls, d_ok, w.rpk, w.rst);
}

// Pairing checks with a key per item, item i against hash point h_idx[i] (or
// i): e(key_i, H) e(-g1, sg_i) == 1; G1 signatures: e(H, key_i) e(-sg_i, g2) == 1.
pairing_job item_key_job(dgpu_ctx* c, const recover_walk& w, size_t n, const uint32_t* h_idx, const uint32_t* sg,
                         const uint32_t* keys, uint8_t* st) {
  return {.consts = c->eng_consts.u32(),
          .n = n,
          .h = w.h,
          .sg = sg,
          .st = st,
          .h_stride = w.n_rounds,
          .h_idx = h_idx,
          .pk_items = w.g1 ? nullptr : keys,
          .g1form_keys = w.g1 ? keys : nullptr};
}

// VerifyRecovered of every round: e(C_0, H(msg)) e(-g1, sig) == 1 with
// k_recover_select's per-round copy of C_0; G1 signatures:
// e(H(msg), C_0) e(-sig, g2) == 1 over the group key's fixed-Q line table
// (the per-round copy is not used on that side).
pairing_job verify_recovered_job(dgpu_ctx* c, const recover_walk& w) {
  if (w.g1)
    return {.consts = c->grp_key.consts.u32(),
            .n = w.n_rounds,
            .h = w.h,
            .sg = w.rpts,
            .st = w.rst,
            .fixed_table = c->grp_key.table.u32()};
  return item_key_job(c, w, w.n_rounds, nullptr, w.rpts, w.rpk, w.rst);
}

// Exact per-partial recovery over device buffers: VerifyPartial of every
// partial, selection, Lagrange + MSM, VerifyRecovered -- the reference's
// walk, pairing by pairing.  d_ok: one byte per round (1 = recovered and
// VerifyRecovered passed); d_status (optional): ST_* of every partial item.
int recover_exact_locked(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs, size_t m, const uint8_t* d_parts,
                         size_t stride, const uint32_t* d_plen, uint8_t* d_out, uint8_t* d_ok, uint8_t* d_status,
                         hipStream_t s) {
  recover_walk w;
  int rc;
  if ((rc = recover_begin_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, true, s, &w))) return rc;
  // VerifyPartial of every partial on the engine
  if ((rc = eng_pairing_locked(c, item_key_job(c, w, w.items, w.hidx, w.sg, w.keys, w.st), s))) return rc;
  const bool wide = walk_wide(w);
  mark(c, s, "recover_select");
  if (wide)
    RC_TRY(recover_walk_wide_launch(c, w, true, 0, d_out, d_ok, s));
  else
    RC_TRY(launch_n(k_recover_select, n_rounds, 64, s, n_rounds, m, w.t, w.idx, w.st, w.sel, w.xs, d_out, d_ok,
                    c->grp_commits.u32(), w.rpts, w.rpk, w.rst));
  mark(c, s, "recover_lagrange");
  if (wide)
    RC_TRY(recover_lagrange_wide_launch(w, d_ok, 0, s));
  else
    RC_TRY(launch_n(k_recover_lagrange, n_rounds * RECOVER_MAX_T, 256, s, n_rounds, w.t, d_ok, w.xs, w.dig, 0));
  mark(c, s, "recover_msm");
  if ((rc = wide   ? recover_msm_wide_locked(c, w, d_ok, 4, s)
            : w.g1 ? recover_msm_g1_locked(c, w, d_ok, 4, s)
                   : recover_msm_w4_launch(w, d_ok, s)) ||
      (rc = recover_finish_launch(w, d_ok, d_out, 4, s)) || (rc = eng_pairing_locked(c, verify_recovered_job(c, w), s)))
    return rc;
  mark(c, s, "recover_verdict");
  RC_TRY(launch_n(k_recover_verdict, n_rounds, 256, s, n_rounds, w.rst, d_out, d_ok));
  if (d_status) HIP_TRY(hipMemcpyAsync(d_status, w.st, w.items, hipMemcpyDeviceToDevice, s));
  mark(c, s);
  return DGPU_OK;
}

// Recovery over device buffers (the body of every recover entry point):
// the batched check (recover.cuh) for every round it decides, the exact
// per-partial path for the rest (compacted, then scattered back).
int recover_slots_locked(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs, size_t m, const uint8_t* d_parts,
                         size_t stride, const uint32_t* d_plen, uint8_t* d_out, uint8_t* d_ok, uint8_t* d_status,
                         hipStream_t s) {
  if (!c->grp_t) return set_err(DGPU_ENOKEY, "no threshold group installed (dgpu_set_group)");
  call_reset(c);
  if (c->recover_exact)
    return recover_exact_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, d_out, d_ok, d_status, s);
  // fresh, unpredictable coefficients per call (partials come from peers)
  std::random_device rd;
  uint64_t seed = ((uint64_t)rd() << 32) ^ rd();
  if (!seed) seed = 1;
  recover_walk w;
  int rc;
  if ((rc = recover_begin_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, false, s, &w))) return rc;
  const bool wide = walk_wide(w);
  mark(c, s, "recover_select");
  if (wide)
    RC_TRY(recover_walk_wide_launch(c, w, false, d_status ? 1 : 0, d_out, d_ok, s));
  else
    RC_TRY(launch_n(k_recover_cand, n_rounds, 64, s, n_rounds, m, w.t, d_status ? 1 : 0, w.idx, w.st, w.sel, w.xs, w.cls,
                    d_ok, d_out));
  mark(c, s, "recover_lagrange");
  if (wide)
    RC_TRY(recover_lagrange_wide_launch(w, d_ok, seed, s));
  else
    RC_TRY(launch_n(k_recover_lagrange, n_rounds * RECOVER_MAX_T, 256, s, n_rounds, w.t, d_ok, w.xs, w.dig, seed));
  mark(c, s, "recover_msm");
  if ((rc = wide   ? recover_msm_wide_locked(c, w, d_ok, 5, s)
            : w.g1 ? recover_msm_g1_locked(c, w, d_ok, 5, s)
                   : recover_msm_g2_locked(c, w, d_ok, s)) ||
      (rc = recover_finish_launch(w, d_ok, d_out, 5, s)) || (rc = recover_combine_launch(c, w, d_ok, s)))
    return rc;
  // one pairing per round: e(A, H) e(-g1, B) == 1; G1 signatures: e(H, A) e(-B, g2) == 1
  if ((rc = eng_pairing_locked(c, item_key_job(c, w, n_rounds, nullptr, w.rpts, w.rpk, w.rst), s))) return rc;
  mark(c, s, "recover_verdict");
  RC_TRY(launch_n(k_recover_rlc_verdict, n_rounds, 256, s, n_rounds, d_status ? 1 : 0, w.rst, w.cls, d_ok, d_out));
  if (d_status) HIP_TRY(hipMemcpyAsync(d_status, w.st, w.items, hipMemcpyDeviceToDevice, s));
  // rounds left to the exact path
  std::vector<uint8_t> hc(n_rounds);
  HIP_TRY(hipMemcpyAsync(hc.data(), w.cls, n_rounds, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<uint32_t> list;
  for (size_t r = 0; r < n_rounds; ++r)
    if ((hc[r] & 0x0F) == REC_EXACT) list.push_back((uint32_t)r);
  mark(c, s);
  const size_t nx = list.size();
  if (nx == 0) return DGPU_OK;
  const size_t xi = nx * m;
  if ((rc = c->rec_x_list.ensure(nx * 4)) || (rc = c->rec_x_msgs.ensure(nx * 32)) ||
      (rc = c->rec_x_parts.ensure(xi * stride)) || (rc = c->rec_x_plen.ensure(xi * 4)) ||
      (rc = c->rec_x_out.ensure(nx * 96)) || (rc = c->rec_x_ok.ensure(nx)) || (rc = c->rec_x_st.ensure(xi)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->rec_x_list.p, list.data(), nx * 4, hipMemcpyHostToDevice, s));
  const uint32_t* const x_list = c->rec_x_list.u32();
  uint8_t *const x_msgs = c->rec_x_msgs.u8(), *const x_parts = c->rec_x_parts.u8(), *const x_out = c->rec_x_out.u8(),
                 *const x_ok = c->rec_x_ok.u8(), *const x_st = c->rec_x_st.u8();
  uint32_t* const x_plen = c->rec_x_plen.u32();
  RC_TRY(launch_n(k_gather_rounds, xi, 256, s, nx, x_list, m, stride, d_msgs, d_parts, d_plen, x_msgs, x_parts, x_plen));
  if ((rc = recover_exact_locked(c, nx, x_msgs, m, x_parts, stride, x_plen, x_out, x_ok, x_st, s))) return rc;
  return launch_n(k_scatter_rounds, xi, 256, s, nx, x_list, m, x_out, x_ok, x_st, d_out, d_ok, d_status);
}

// recover_slots_locked works on 96-byte round slots (its selection, verdict
// and scatter kernels zero and copy whole slots); a G1-signature group's
// 48-byte signatures are packed from the context's slots to d_out + 48 r.
int recover_device_locked(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs, size_t m, const uint8_t* d_parts,
                          size_t stride, const uint32_t* d_plen, uint8_t* d_out, uint8_t* d_ok, uint8_t* d_status,
                          hipStream_t s) {
  if (!c->grp_g1) return recover_slots_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, d_out, d_ok, d_status, s);
  int rc;
  if ((rc = c->rec_slots.ensure(n_rounds * 96))) return rc;
  uint8_t* slots = c->rec_slots.u8();
  if ((rc = recover_slots_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, slots, d_ok, d_status, s))) return rc;
  return launch_n(k_recover_pack48, n_rounds * 48, 256, s, n_rounds, slots, d_ok, d_out);
}

}  // namespace

extern "C" {

int dgpu_recover_batch_device(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs32, size_t m,
                              const uint8_t* d_partials, size_t partial_stride, const uint32_t* d_partial_len,
                              uint8_t* d_out_sigs, uint8_t* d_ok, uint8_t* d_status, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (n_rounds == 0) return DGPU_OK;  // an empty batch: no-op, NULL buffers accepted (as the verify entry points)
  if (!d_msgs32 || !d_partials || !d_partial_len || !d_out_sigs || !d_ok) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (m == 0 || partial_stride < group_partial_bytes(c))
    return set_err(DGPU_EINVAL, "need m >= 1 partial slots and stride >= %zu", group_partial_bytes(c));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  return recover_device_locked(c, n_rounds, d_msgs32, m, d_partials, partial_stride, d_partial_len, d_out_sigs,
                               d_ok, d_status, s);
}

int dgpu_recover_batch(dgpu_ctx* c, size_t n_rounds, const uint8_t* msgs32, size_t m, const uint8_t* partials,
                       size_t partial_stride, const uint32_t* partial_len, uint8_t* out_sigs, uint8_t* ok_bits,
                       uint8_t* partial_valid) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (n_rounds == 0) return DGPU_OK;  // an empty batch: no-op, NULL buffers accepted (as the verify entry points)
  if (!msgs32 || !partials || !partial_len || !out_sigs || !ok_bits) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (m == 0 || partial_stride < group_partial_bytes(c))
    return set_err(DGPU_EINVAL, "need m >= 1 partial slots and stride >= %zu", group_partial_bytes(c));
  if (!c->grp_t) return set_err(DGPU_ENOKEY, "no threshold group installed (dgpu_set_group)");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  const size_t items = n_rounds * m;
  for (size_t i = 0; i < items; ++i)
    if (partial_len[i] > partial_stride) return set_err(DGPU_EINVAL, "partial_len[%zu] > stride", i);
  int rc;
  if ((rc = c->rec_msgs.ensure(n_rounds * 32))) return rc;
  if ((rc = c->rec_parts.ensure(items * partial_stride))) return rc;
  if ((rc = c->rec_plen.ensure(items * 4))) return rc;
  if ((rc = c->rec_out.ensure(n_rounds * 96))) return rc;
  if ((rc = c->rec_ok.ensure(n_rounds))) return rc;
  if ((rc = c->out_reason.ensure(items))) return rc;
  HIP_TRY(hipMemcpyAsync(c->rec_msgs.p, msgs32, n_rounds * 32, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->rec_parts.p, partials, items * partial_stride, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->rec_plen.p, partial_len, items * 4, hipMemcpyHostToDevice, s));
  if ((rc = recover_device_locked(c, n_rounds, c->rec_msgs.u8(), m, c->rec_parts.u8(), partial_stride, c->rec_plen.u32(),
                                  c->rec_out.u8(), c->rec_ok.u8(), partial_valid ? c->out_reason.u8() : nullptr, s)))
    return rc;
  std::vector<uint8_t> okv(n_rounds), stv(partial_valid ? items : 0);
  HIP_TRY(hipMemcpyAsync(out_sigs, c->rec_out.p, n_rounds * group_sig_bytes(c), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(okv.data(), c->rec_ok.p, n_rounds, hipMemcpyDeviceToHost, s));
  if (partial_valid) HIP_TRY(hipMemcpyAsync(stv.data(), c->out_reason.p, items, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memset(ok_bits, 0, (n_rounds + 7) / 8);
  for (size_t r = 0; r < n_rounds; ++r)
    if (okv[r]) ok_bits[r >> 3] |= (uint8_t)(1u << (r & 7));
  if (partial_valid)
    for (size_t i = 0; i < items; ++i) partial_valid[i] = stv[i] == ST_OK;
  return DGPU_OK;
}

// ---------------------------------------------------------------- partial signing (data tool)
int dgpu_make_partials(dgpu_ctx* c, size_t n_rounds, const uint8_t* msgs32, size_t m, const uint32_t* sign_idx,
                       const uint32_t* label, const uint8_t* shares_be32, size_t n_shares, uint8_t* out98) {
  return dgpu_make_partials_scheme(c, DGPU_SCHEME_CHAINED, n_rounds, msgs32, m, sign_idx, label, shares_be32, n_shares,
                                   out98);
}

int dgpu_make_partials_scheme(dgpu_ctx* c, int scheme, size_t n_rounds, const uint8_t* msgs32, size_t m,
                              const uint32_t* sign_idx, const uint32_t* label, const uint8_t* shares_be32,
                              size_t n_shares, uint8_t* out98) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  const bool g1 = sig_on_g1(scheme);
  const size_t pb = g1 ? 50 : 98;  // bytes per partial
  if (n_rounds == 0 || m == 0) return DGPU_OK;
  if (!msgs32 || !sign_idx || !label || !shares_be32 || !out98) return set_err(DGPU_EINVAL, "null argument");
  const size_t items = n_rounds * m;
  for (size_t i = 0; i < items; ++i)
    if (sign_idx[i] >= n_shares || label[i] > 0xFFFF) return set_err(DGPU_EINVAL, "bad share index at item %zu", i);
  std::vector<scalar256> sh(n_shares);
  for (size_t j = 0; j < n_shares; ++j) sh[j] = scalar_from_be32(shares_be32 + 32 * j);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  int rc;
  stream_scratch<6> tmp(s);
  DevBuf &d_msgs = tmp.b[0], &d_h = tmp.b[1], &d_si = tmp.b[2], &d_lb = tmp.b[3], &d_sh = tmp.b[4], &d_out = tmp.b[5];
  if ((rc = d_msgs.ensure(n_rounds * 32)) || (rc = d_h.ensure(n_rounds * G2A_WORDS * 4)) ||
      (rc = d_si.ensure(items * 4)) || (rc = d_lb.ensure(items * 4)) || (rc = d_sh.ensure(n_shares * sizeof(scalar256))) ||
      (rc = d_out.ensure(items * pb)))
    return rc;
  hipError_t e = hipMemcpyAsync(d_msgs.p, msgs32, n_rounds * 32, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_si.p, sign_idx, items * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_lb.p, label, items * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_sh.p, sh.data(), n_shares * sizeof(scalar256), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return set_err(DGPU_EDEVICE, "make_partials: %s", hipGetErrorString(e));
  if ((rc = recover_hash_launch(g1, scheme == DGPU_SCHEME_G1_RFC9380 ? 1 : 0, n_rounds, d_msgs.u8(), d_h.u32(), s)) ||
      (rc = launch_n(g1 ? k_sign_partials_g1 : k_sign_partials, items, 64, s, items, m, n_rounds, d_h.u32(), d_si.u32(),
                     d_lb.u32(), d_sh.as<scalar256>(), d_out.u8())))
    return rc;
  e = hipMemcpyAsync(out98, d_out.p, items * pb, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return set_err(DGPU_EDEVICE, "make_partials: %s", hipGetErrorString(e));
  return DGPU_OK;
}

}  // extern "C"
