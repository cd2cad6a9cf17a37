// Host code behind the per-record-key entry points of the C ABI:
// dgpu_verify_keyed[_device] (a key table and a key index per record) and
// dgpu_verify_partials[_device] (VerifyPartial of every slot under the installed
// group, the item key PubPoly.Eval(index)).  Included by capi.hip behind
// threshold_host.h (one translation unit: the kernels, the context and the
// recovery prologue live there).
//
// Per-record mode: both front ends end in one eng_pairing_locked call with a
// key per item (pairing_job::pk_items / g1form_keys), on one stream.
// RLC mode (n >= DGPU_RLC_MIN items): both front ends hand their points, group
// ids and per-item keys to keyed_rlc_locked, one random linear combination and
// one 2-pairing check per key (keyed.cuh); the items of a failing key are
// then checked one by one.

namespace {

size_t keyed_key_words(bool g2key) { return g2key ? (size_t)G2A_WORDS : 2 * (size_t)FP_LIMBS; }

// The arguments every keyed form shares, before any device work.
int keyed_check_args(int scheme, size_t n_keys, size_t key_len, int mode) {
  if (!scheme_known(scheme)) return set_err(DGPU_EINVAL, "bad scheme %d", scheme);
  if (mode != DGPU_MODE_PER_ROUND && mode != DGPU_MODE_RLC) return set_err(DGPU_EINVAL, "bad mode %d", mode);
  const size_t want = sig_on_g1(scheme) ? 96 : 48;
  if (key_len != want)
    return set_err(DGPU_EINVAL, "keys of scheme %d are %zu bytes (compressed %s), got %zu", scheme, want,
                   sig_on_g1(scheme) ? "G2" : "G1", key_len);
  if (n_keys < 1 || n_keys > KEYED_MAX_KEYS)
    return set_err(DGPU_EINVAL, "n_keys=%zu outside [1, %zu]", n_keys, KEYED_MAX_KEYS);
  return DGPU_OK;
}

// The call's key table (host) decoded on the device, asynchronous on s.  The
// bytes leave the caller's buffer before this returns: they go through a
// pinned copy the context owns, reused once the previous keyed call's upload
// has read it.
int keyed_table_locked(dgpu_ctx* c, bool g2key, size_t n_keys, const uint8_t* keys, size_t key_len, hipStream_t s,
                       keyed_table_layout* T) {
  int rc = carve(c->ky_tab, T, n_keys, key_len);
  if (rc) return rc;
  const size_t bytes = n_keys * key_len;
  if (!c->ky_ev) HIP_TRY(hipEventCreateWithFlags(&c->ky_ev, hipEventDisableTiming));
  if (c->ky_ev_used) HIP_TRY(hipEventSynchronize(c->ky_ev));
  if (bytes > c->ky_host_cap) {
    if (c->ky_host) HIP_TRY(hipHostFree(c->ky_host));
    c->ky_host = nullptr, c->ky_host_cap = 0;
    HIP_TRY(hipHostMalloc(&c->ky_host, bytes, hipHostMallocDefault));
    c->ky_host_cap = bytes;
  }
  memcpy(c->ky_host, keys, bytes);
  mark(c, s, "keyed_keys");
  HIP_TRY(hipMemcpyAsync(T->in, c->ky_host, bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(c->ky_ev, s));
  c->ky_ev_used = true;
  return launch_n(g2key ? k_decode_commits_g2 : k_decode_commits, n_keys, 64, s, (int)n_keys, T->in, T->pts, T->rc);
}

// One pairing batch of m items with a key per item (g2key: G1 signatures).
// The signatures behind these items were subgroup-checked at decode.
pairing_job keyed_items_job(dgpu_ctx* c, bool g2key, size_t m, const uint32_t* h, const uint32_t* sg,
                            const uint32_t* keys, uint8_t* st) {
  return {.consts = c->eng_consts.u32(),
          .n = m,
          .h = h,
          .sg = sg,
          .st = st,
          .pk_items = g2key ? nullptr : keys,
          .g1form_keys = g2key ? keys : nullptr};
}

// What the two front ends hand to the RLC core (device pointers): n items,
// item i in group gid[i] (an item with gid[i] >= n_groups is not combined and
// goes to the exact check), hash point h_idx[i] (null: i) of an affine SoA of
// stride h_stride, signature points and per-item keys (the engine's per-item
// layout) of stride n, and the statuses: every final verdict (decode,
// subgroup, infinity, ST_KEY) and ST_OK for the undecided items.  Every item
// of a group carries the same key.
struct keyed_rlc_in {
  size_t n, n_groups;
  uint64_t seed;
  const uint32_t* gid;
  const uint32_t* h;
  size_t h_stride;
  const uint32_t* h_idx;
  const uint32_t* sg;
  const uint32_t* item_keys;
  uint8_t* st;
};

// RLC mode behind the hash, the (subgroup-checking) decode and the per-item
// keys: leaves, grouping by key, load-balanced per-key sums, one node check
// per non-empty key, then the exact check of the failing keys' items (one
// stream synchronisation to size it).
template <class Gr>
int keyed_rlc_t(dgpu_ctx* c, const keyed_rlc_in& in, hipStream_t s) {
  using M = GrMem<Gr>;
  constexpr bool G2KEY = std::is_same<Gr, G1Ops>::value;  // G1 signatures: G2 keys
  const unsigned B = 256;
  const size_t n = in.n, n_keys = in.n_groups;
  const uint32_t ng = (uint32_t)n_keys;
  const int kw = (int)keyed_key_words(G2KEY);
  const size_t R = keyed_range_len(n, c->keyed_range), NT = keyed_ranges(n, R), m = std::min(n_keys, n);
  const uint32_t *const h = in.h, *const sg = in.sg, *const d_key_idx = in.gid, *const item_keys = in.item_keys;
  uint8_t* const st = in.st;
  keyed_rlc_layout K;
  int rc = carve(c->ky_rlc, &K, n, n_keys, NT, m, M::AFF, M::JAC, kw);
  if (rc) return rc;
  mark(c, s, "keyed_leaves");
  RC_TRY(launch_n(k_keyed_leaves<Gr>, 2 * n, B, s, n, in.seed, h, in.h_stride, in.h_idx, sg, st, K.leaf_p, K.leaf_s));
  mark(c, s, "keyed_group");
  HIP_TRY(hipMemsetAsync(K.counts, 0, n_keys * 4, s));
  HIP_TRY(hipMemsetAsync(K.nfail, 0, 4, s));
  RC_TRY(launch_n(k_keyed_count, n, B, s, n, ng, d_key_idx, st, K.counts));
  RC_TRY(launch(k_keyed_scan, dim3(1), dim3(KEYED_SCAN_THREADS), s, ng, K.counts, K.offsets, K.cursor, K.cpos, K.totals));
  RC_TRY(launch_n(k_keyed_scatter, n, B, s, n, ng, d_key_idx, st, K.cursor, K.list, K.lkey));
  mark(c, s, "keyed_sums");
  RC_TRY(launch_n(k_keyed_sums<Gr>, 2 * NT, B, s, NT, R, K.totals, ng, K.offsets, K.counts, K.list, K.lkey, n, K.leaf_p,
                  K.leaf_s, K.sums, K.part));
  RC_TRY(launch(k_keyed_fixup<Gr>, dim3((unsigned)(2 * n_keys)), dim3(64), s, NT, R, ng, K.offsets, K.counts, K.part,
                K.sums));
  mark(c, s, "keyed_prep");
  // the slots past the non-empty keys: trivial candidates with zero points
  HIP_TRY(hipMemsetAsync(K.ch, 0, (size_t)M::AFF * m * 4, s));
  HIP_TRY(hipMemsetAsync(K.cs, 0, (size_t)M::AFF * m * 4, s));
  HIP_TRY(hipMemsetAsync(K.ckeys, 0, (size_t)kw * m * 4, s));
  HIP_TRY(hipMemsetAsync(K.cst, RLC_TRIVIAL, m, s));
  RC_TRY(launch_n(k_keyed_prep<Gr>, n_keys, 64, s, ng, m, K.counts, K.cpos, K.offsets, K.list, K.sums, n, item_keys, kw,
                  K.ch, K.cs, K.ckeys, K.cst));
  if ((rc = eng_pairing_locked(c, keyed_items_job(c, G2KEY, m, K.ch, K.cs, K.ckeys, K.cst), s))) return rc;
  // the records of the failing keys, one by one
  RC_TRY(launch_n(k_keyed_list_failing, n, B, s, n, ng, d_key_idx, st, K.cpos, K.cst, K.flist, K.nfail));
  uint32_t nf = 0;
  HIP_TRY(hipMemcpyAsync(&nf, K.nfail, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (nf == 0) return DGPU_OK;
  if (nf > n) return set_err(DGPU_EDEVICE, "keyed RLC: %u listed records of %zu", nf, n);
  keyed_exact_layout X;
  if ((rc = carve(c->ky_exact, &X, (size_t)nf, M::AFF, kw))) return rc;
  mark(c, s, "keyed_fallback");
  RC_TRY(launch_n(k_keyed_compact, nf, B, s, nf, K.flist, n, h, in.h_stride, in.h_idx, sg, M::AFF, item_keys, kw, X.h, X.s,
                  X.keys, X.st));
  if ((rc = eng_pairing_locked(c, keyed_items_job(c, G2KEY, nf, X.h, X.s, X.keys, X.st), s))) return rc;
  mark(c, s, "keyed_fallback");
  return launch_n(k_keyed_scatter_verdicts, nf, B, s, nf, K.flist, X.st, st);
}

int keyed_rlc_locked(dgpu_ctx* c, bool g1, const keyed_rlc_in& in, hipStream_t s) {
  return with_group(g1, [&](auto gr) { return keyed_rlc_t<GROUP_OF(gr)>(c, in, s); });
}

// Everything up to the per-record status of a keyed call over device records
// (a: raw messages and signatures; d_key_idx: the records' key indices), on
// the one stream s: the key table, the hash and the signature decode of the
// single-key per-round path, the gather of the per-item keys (ST_KEY), one
// pairing batch with a key per item.
int keyed_status_locked(dgpu_ctx* c, const verify_args& a, size_t n_keys, const uint8_t* keys, size_t key_len,
                        const uint32_t* d_key_idx, hipStream_t s) {
  const unsigned B = 256;
  const size_t n = a.n;
  const bool g1 = sig_on_g1(a.scheme);
  int rc;
  call_reset(c);
  const bool rlc = a.mode == DGPU_MODE_RLC && n >= c->rlc_min;
  keyed_table_layout T;
  if ((rc = c->status.ensure(n)) || (rc = c->ky_keys.ensure(n * keyed_key_words(g1) * 4)) ||
      (rc = keyed_table_locked(c, g1, n_keys, keys, key_len, s, &T)))
    return rc;
  uint8_t* st = c->status.u8();
  uint32_t* item_keys = c->ky_keys.u32();
  lane_scratch& L = c->lane[0];
  if ((rc = g1 ? g1_hash_decode_locked(c, a, st, s, false)
               : g2_lane_hash_locked(c, L, n, a.m, a.sigs, a.sig_stride, a.sig_len, st, s, nullptr, nullptr, nullptr, 0,
                                     rlc)))
    return rc;
  mark(c, s, "keyed_gather");
  RC_TRY(launch_n(g1 ? k_keyed_gather<true> : k_keyed_gather<false>, n, B, s, n, n_keys, d_key_idx, T.pts, T.rc, item_keys,
                  st));
  if (rlc)
    return keyed_rlc_locked(c, g1, {n, n_keys, a.seed, d_key_idx, L.h_pts.u32(), n, nullptr, L.sig_pts.u32(), item_keys, st},
                            s);
  return eng_pairing_locked(c,
                            {.consts = c->eng_consts.u32(),
                             .n = n,
                             .h = L.h_pts.u32(),
                             .sg = L.sig_pts.u32(),
                             .st = st,
                             .pk_items = g1 ? nullptr : item_keys,
                             .sig_subgroup = !g1 && !c->decode_subgroup,
                             .g1form_keys = g1 ? item_keys : nullptr},
                            s);
}

// VerifyPartial of every slot over device buffers: the first step of
// recover_exact_locked (the prologue, then one pairing per partial against its
// share key), then the verdict pack.  RLC mode at DGPU_RLC_MIN slots and above:
// the keyed core with the share index as the group id (the group's table
// size groups; an index above it, whose key was evaluated on the fly, goes to
// the exact check), the round's hash point through the item -> round map and
// the share keys the decoder left per item (its signature decoders check the
// subgroup).  d_reason (optional): ST_* per slot.
int verify_partials_locked(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs, size_t m, const uint8_t* d_parts,
                           size_t stride, const uint32_t* d_plen, int mode, uint64_t seed, uint8_t* d_bits,
                           uint8_t* d_reason, hipStream_t s) {
  call_reset(c);
  recover_walk w;
  int rc;
  if ((rc = recover_begin_locked(c, n_rounds, d_msgs, m, d_parts, stride, d_plen, true, s, &w))) return rc;
  if (mode == DGPU_MODE_RLC && w.items >= c->rlc_min)
    rc = keyed_rlc_locked(c, w.g1, {w.items, (size_t)c->grp_n, seed, w.idx, w.h, n_rounds, w.hidx, w.sg, w.keys, w.st}, s);
  else
    rc = eng_pairing_locked(c, item_key_job(c, w, w.items, w.hidx, w.sg, w.keys, w.st), s);
  if (rc) return rc;
  mark(c, s, "pack_verdicts");
  RC_TRY(launch_n(k_pack_verdicts, (w.items + 7) / 8, 256, s, w.items, w.st, d_bits));
  mark(c, s);
  if (d_reason) HIP_TRY(hipMemcpyAsync(d_reason, w.st, w.items, hipMemcpyDeviceToDevice, s));
  return DGPU_OK;
}

// The arguments both partial forms share (n_rounds > 0), before any device work.
int partials_check_args(const dgpu_ctx* c, size_t m, size_t stride) {
  if (!c->grp_t) return set_err(DGPU_ENOKEY, "no threshold group installed (dgpu_set_group)");
  if (m == 0 || stride < group_partial_bytes(c))
    return set_err(DGPU_EINVAL, "need m >= 1 partial slots and stride >= %zu", group_partial_bytes(c));
  return DGPU_OK;
}

}  // namespace

extern "C" {

int dgpu_verify_keyed_device(dgpu_ctx* c, int scheme, size_t n_keys, const uint8_t* keys, size_t key_len, size_t n,
                             const uint32_t* d_key_idx, const uint8_t* d_msgs, size_t msg_stride,
                             const uint32_t* d_msg_len, const uint8_t* d_sigs, size_t sig_stride,
                             const uint32_t* d_sig_len, int mode, uint64_t rlc_seed, uint8_t* d_bits, uint8_t* d_reason,
                             void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = keyed_check_args(scheme, n_keys, key_len, mode);
  if (rc || n == 0) return rc;
  if (!keys || !d_key_idx || !d_msg_len || (!d_msgs && msg_stride) || !d_sigs || !d_sig_len || !d_bits)
    return set_err(DGPU_EINVAL, "null argument");
  if (sig_stride < (sig_on_g1(scheme) ? 48u : 96u)) return set_err(DGPU_EINVAL, "bad signature stride");
  if (n > 0xFFFFFFFFull) return set_err(DGPU_EINVAL, "batch too large (%zu records)", n);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  // (a zero stride never dereferences the message pointer; the source is "raw" by its non-null value)
  const verify_args a{scheme, n, raw_src(d_msgs ? d_msgs : (const uint8_t*)d_msg_len, msg_stride, d_msg_len), d_sigs,
                      sig_stride, d_sig_len, mode, rlc_seed};
  if ((rc = keyed_status_locked(c, a, n_keys, keys, key_len, d_key_idx, s))) return rc;
  return results_out_locked(c, a, d_bits, nullptr, d_reason, hipMemcpyDeviceToDevice, nullptr, s);
}

int dgpu_verify_keyed(dgpu_ctx* c, int scheme, size_t n_keys, const uint8_t* keys, size_t key_len, size_t n,
                      const uint32_t* key_idx, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                      const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len, int mode, uint64_t rlc_seed,
                      uint8_t* verdict_bits, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  int rc = keyed_check_args(scheme, n_keys, key_len, mode);
  if (rc || n == 0) return rc;
  if (!keys || !key_idx || !msg_len || (!msgs && msg_stride) || !sigs || !sig_len || !verdict_bits)
    return set_err(DGPU_EINVAL, "null argument");
  if (sig_stride < (sig_on_g1(scheme) ? 48u : 96u)) return set_err(DGPU_EINVAL, "bad signature stride");
  if (n > 0xFFFFFFFFull) return set_err(DGPU_EINVAL, "batch too large (%zu records)", n);
  for (size_t i = 0; i < n; ++i)
    if (key_idx[i] >= n_keys) return set_err(DGPU_EINVAL, "key_idx[%zu]=%u >= n_keys", i, key_idx[i]);
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  static const uint8_t empty = 0;
  verify_args a{scheme, n, raw_src(msgs ? msgs : &empty, msg_stride, msg_len), sigs, sig_stride, sig_len, mode,
                rlc_seed};
  // (always the ring: the A/B build's DGPU_STAGE=pageable applies to the record list's own staging in
  // verify_host_locked, and the key indices have no pageable path)
  // the records through the pinned ring in one slice (a's pointers become the device copies'), the key indices
  // behind them on the copy stream: one more 4-byte array, counted with the records
  if ((rc = c->in_key_idx.ensure(n * 4)) || (rc = stage_all_host_locked(c, a, s)) ||
      (rc = ring_copy_locked(c, c->in_key_idx.p, key_idx, n * 4)))
    return rc;
  HIP_TRY(hipStreamWaitEvent(s, c->ring_ev[c->ring_next ^ 1], 0));  // the copy stream is in order: its last DMA
  c->last_stage_bytes += n * 4;
  if ((rc = keyed_status_locked(c, a, n_keys, keys, key_len, c->in_key_idx.u32(), s)) ||
      (rc = results_out_locked(c, a, nullptr, verdict_bits, reason, hipMemcpyDeviceToHost, nullptr, s)))
    return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

int dgpu_verify_partials_device(dgpu_ctx* c, size_t n_rounds, const uint8_t* d_msgs32, size_t m,
                                const uint8_t* d_partials, size_t partial_stride, const uint32_t* d_partial_len,
                                int mode, uint64_t rlc_seed, uint8_t* d_valid_bits, uint8_t* d_reason, void* stream) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (mode != DGPU_MODE_PER_ROUND && mode != DGPU_MODE_RLC) return set_err(DGPU_EINVAL, "bad mode %d", mode);
  if (n_rounds == 0) return DGPU_OK;  // an empty batch: no-op, NULL buffers accepted
  if (!d_msgs32 || !d_partials || !d_partial_len || !d_valid_bits) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  int rc = partials_check_args(c, m, partial_stride);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = caller_stream(stream);
  stream_order ord(c, s);
  return verify_partials_locked(c, n_rounds, d_msgs32, m, d_partials, partial_stride, d_partial_len, mode, rlc_seed,
                                d_valid_bits, d_reason, s);
}

int dgpu_verify_partials(dgpu_ctx* c, size_t n_rounds, const uint8_t* msgs32, size_t m, const uint8_t* partials,
                         size_t partial_stride, const uint32_t* partial_len, int mode, uint64_t rlc_seed,
                         uint8_t* valid_bits, uint8_t* reason) {
  if (!c) return set_err(DGPU_EINVAL, "null ctx");
  if (mode != DGPU_MODE_PER_ROUND && mode != DGPU_MODE_RLC) return set_err(DGPU_EINVAL, "bad mode %d", mode);
  if (n_rounds == 0) return DGPU_OK;  // an empty batch: no-op, NULL buffers accepted
  if (!msgs32 || !partials || !partial_len || !valid_bits) return set_err(DGPU_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  int rc = partials_check_args(c, m, partial_stride);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  stream_order ord(c, s);
  const size_t items = n_rounds * m;
  if ((rc = c->rec_msgs.ensure(n_rounds * 32)) || (rc = c->rec_parts.ensure(items * partial_stride)) ||
      (rc = c->rec_plen.ensure(items * 4)) || (rc = c->out_bits.ensure((items + 7) / 8)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->rec_msgs.p, msgs32, n_rounds * 32, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->rec_parts.p, partials, items * partial_stride, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->rec_plen.p, partial_len, items * 4, hipMemcpyHostToDevice, s));
  if ((rc = verify_partials_locked(c, n_rounds, c->rec_msgs.u8(), m, c->rec_parts.u8(), partial_stride, c->rec_plen.u32(),
                                   mode, rlc_seed, c->out_bits.u8(), nullptr, s)))
    return rc;
  HIP_TRY(hipMemcpyAsync(valid_bits, c->out_bits.p, (items + 7) / 8, hipMemcpyDeviceToHost, s));
  if (reason) HIP_TRY(hipMemcpyAsync(reason, c->status.p, items, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DGPU_OK;
}

}  // extern "C"
