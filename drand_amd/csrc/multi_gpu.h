// Multi-GPU batch verification behind the C ABI (dgpu_multi_open /
// dgpu_verify_multi).  Included at the end of capi.hip
// (one translation unit: the kernels and the context live there).
//
// The reference's bulk caller walks the chain serially
// (chain/beacon/sync_manager.go:188-222); every stored beacon carries its own
// PreviousSig (chain/beacon.go:15), so round verdicts are independent and the
// batch shards into contiguous round ranges, one per GPU, with no data-path
// collective.  RCCL over xGMI moves only results:
//  - per-round mode: one all-gather of the per-device verdict bitmaps (and
//    reason bytes) -- shards are multiples of 8 rounds, so the gathered
//    bitmaps concatenate into the batch's bitmap;
//  - RLC mode: one all-gather of the per-device RLC roots (two Jacobian sums
//    of the signature group: 672 bytes for G2 signatures, 336 for the G1
//    schemes; each computed by bucket MSM, rlc_msm.cuh), summed on
//    device 0 and checked there with a single pairing (one final
//    exponentiation for the whole node); only when that fails does each
//    device build its tree of leaves and descend it (root first) to
//    per-round verdicts, and the bitmaps are gathered as in per-round mode.
// RCCL is loaded at dgpu_multi_open (dlopen), so the single-GPU library has
// no link-time dependency on it.
//
// dgpu_verify_segment_multi is the same call over a linked segment (the
// signatures alone, client/verify.go:118-178): there the first round of shard
// k > 0 hashes the last record of shard k - 1, so that one record travels with
// the shard as its halo (kernels.cuh msg_src_halo), staged from the caller's
// own arrays ahead of the shard; everything else is one function
// (multi_verify) over a per-shard message source.
//
// Test mode: with DGPU_MULTI_ALLOW_SAME_DEVICE=1 in the environment a handle
// may list one device several times (devs = {0, 0, 0}: one context each, own
// streams and buffers) and its all-gathers are in-library device copies
// ordered by events instead of RCCL (a communicator cannot hold one device
// twice).  Everything else -- shard bookkeeping, per-device seeds, root sum
// and check on the first context, short / empty shard padding -- is the
// production code path, so a one-GPU box executes the D >= 2 branches.

namespace {

struct rccl_api {
  void* h = nullptr;
  ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
};

int load_rccl(rccl_api& r) {
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* nm : names) {
    r.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    if (r.h) break;
  }
  if (!r.h) return set_err(DGPU_EUNSUPPORTED, "RCCL not found (dlopen librccl.so.1: %s)", dlerror());
  r.comm_init_all = (decltype(r.comm_init_all))dlsym(r.h, "ncclCommInitAll");
  r.comm_destroy = (decltype(r.comm_destroy))dlsym(r.h, "ncclCommDestroy");
  r.all_gather = (decltype(r.all_gather))dlsym(r.h, "ncclAllGather");
  r.group_start = (decltype(r.group_start))dlsym(r.h, "ncclGroupStart");
  r.group_end = (decltype(r.group_end))dlsym(r.h, "ncclGroupEnd");
  r.error_string = (decltype(r.error_string))dlsym(r.h, "ncclGetErrorString");
  if (!r.comm_init_all || !r.comm_destroy || !r.all_gather || !r.group_start || !r.group_end || !r.error_string)
    return set_err(DGPU_EUNSUPPORTED, "RCCL is missing a symbol");
  return DGPU_OK;
}

#define NCCL_TRY(api, expr)                                                                            \
  do {                                                                                                 \
    ncclResult_t _r = (expr);                                                                          \
    if (_r != ncclSuccess) return set_err(DGPU_EDEVICE, "%s: %s", #expr, (api).error_string(_r));    \
  } while (0)

// per-device buffers of the gathers
struct multi_bufs {
  DevBuf bits, reasons, all_bits, all_reasons, root, all_roots;
};

}  // namespace

struct dgpu_multi {
  int ndev = 0;
  std::vector<int> devs;
  std::vector<dgpu_ctx*> ctx;
  std::vector<ncclComm_t> comm;
  std::vector<multi_bufs> buf;
  rccl_api api;
  std::mutex mu;
  bool loopback = false;          // DGPU_MULTI_ALLOW_SAME_DEVICE=1: device copies instead of RCCL (tests)
  std::vector<hipEvent_t> gev;    // loopback: per-device "source ready" events
};

extern "C" {

int dgpu_multi_open(int ndev, const int* devs, dgpu_multi** out) {
  if (!out || !devs || ndev < 1) return set_err(DGPU_EINVAL, "bad arguments");
  *out = nullptr;
  const char* same = getenv("DGPU_MULTI_ALLOW_SAME_DEVICE");
  const bool loopback = same && !strcmp(same, "1");
  for (int i = 0; i < ndev && !loopback; ++i)
    for (int j = 0; j < i; ++j)
      if (devs[i] == devs[j]) return set_err(DGPU_EINVAL, "device %d listed twice", devs[i]);
  dgpu_multi* m = new dgpu_multi();
  m->loopback = loopback;
  int rc = loopback ? DGPU_OK : load_rccl(m->api);
  if (rc) {
    delete m;
    return rc;
  }
  m->ndev = ndev;
  m->devs.assign(devs, devs + ndev);
  m->buf.resize(ndev);
  for (int i = 0; i < ndev; ++i) {
    dgpu_ctx* c = nullptr;
    if ((rc = dgpu_open(devs[i], &c))) {
      std::string msg = g_last_error;
      dgpu_multi_close(m);
      return set_err(rc, "%s", msg.c_str());
    }
    m->ctx.push_back(c);
  }
  if (loopback) {
    m->gev.assign(ndev, nullptr);
    for (int i = 0; i < ndev; ++i) {
      (void)hipSetDevice(devs[i]);
      if (hipEventCreateWithFlags(&m->gev[i], hipEventDisableTiming) != hipSuccess) {
        dgpu_multi_close(m);
        return set_err(DGPU_EDEVICE, "hipEventCreate failed");
      }
    }
    *out = m;
    return DGPU_OK;
  }
  m->comm.resize(ndev);
  ncclResult_t r = m->api.comm_init_all(m->comm.data(), ndev, devs);
  if (r != ncclSuccess) {
    std::string msg = m->api.error_string(r);
    m->comm.clear();
    dgpu_multi_close(m);
    return set_err(DGPU_EDEVICE, "ncclCommInitAll: %s", msg.c_str());
  }
  *out = m;
  return DGPU_OK;
}

void dgpu_multi_close(dgpu_multi* m) {
  if (!m) return;
  for (size_t i = 0; i < m->comm.size(); ++i)
    if (m->comm[i]) m->api.comm_destroy(m->comm[i]);
  for (size_t i = 0; i < m->ctx.size(); ++i) {
    (void)hipSetDevice(m->devs[i]);
    if (i < m->gev.size() && m->gev[i]) (void)hipEventDestroy(m->gev[i]);
    dgpu_close(m->ctx[i]);  // drains the context's streams, which the gathers ran on
  }
  delete m;  // the gather buffers go with the handle
}

int dgpu_multi_context(dgpu_multi* m, int k, dgpu_ctx** out) {
  if (!m || !out || k < 0 || k >= m->ndev) return set_err(DGPU_EINVAL, "bad arguments");
  *out = m->ctx[k];
  return DGPU_OK;
}

}  // extern "C"

namespace {

// Run fn(k) for every device on its own host thread; the first failure's
// code and message become this thread's.
template <class Fn>
int for_each_device(dgpu_multi* m, Fn&& fn) {
  std::vector<int> rcs(m->ndev, DGPU_OK);
  std::vector<std::string> errs(m->ndev);
  std::vector<std::thread> th;
  for (int k = 0; k < m->ndev; ++k)
    th.emplace_back([&, k]() {
      if (hipSetDevice(m->devs[k]) != hipSuccess) {
        rcs[k] = DGPU_EDEVICE;
        errs[k] = "hipSetDevice failed";
        return;
      }
      rcs[k] = fn(k);
      if (rcs[k]) errs[k] = g_last_error;
    });
  for (auto& t : th) t.join();
  for (int k = 0; k < m->ndev; ++k)
    if (rcs[k]) return set_err(rcs[k], "device %d: %s", m->devs[k], errs[k].c_str());
  return DGPU_OK;
}

// One all-gather per device of `bytes` bytes: dst[k] + j * bytes <- src[j]
// for every j, enqueued on each device's stream.  RCCL (one group) or, in
// loopback mode, device copies ordered after every source stream's event.
int multi_all_gather(dgpu_multi* m, const std::vector<const void*>& src, const std::vector<void*>& dst,
                     size_t bytes) {
  const int D = m->ndev;
  if (!m->loopback) {
    NCCL_TRY(m->api, m->api.group_start());
    for (int k = 0; k < D; ++k)
      NCCL_TRY(m->api, m->api.all_gather(src[k], dst[k], bytes, ncclUint8, m->comm[k], m->ctx[k]->stream));
    NCCL_TRY(m->api, m->api.group_end());
    return DGPU_OK;
  }
  for (int j = 0; j < D; ++j) {
    HIP_TRY(hipSetDevice(m->devs[j]));
    HIP_TRY(hipEventRecord(m->gev[j], m->ctx[j]->stream));
  }
  for (int k = 0; k < D; ++k) {
    HIP_TRY(hipSetDevice(m->devs[k]));
    for (int j = 0; j < D; ++j) {
      HIP_TRY(hipStreamWaitEvent(m->ctx[k]->stream, m->gev[j], 0));
      HIP_TRY(hipMemcpyAsync((uint8_t*)dst[k] + (size_t)j * bytes, src[j], bytes, hipMemcpyDeviceToDevice,
                             m->ctx[k]->stream));
    }
  }
  return DGPU_OK;
}

// The final statuses of device k's shard -> its verdict bits and reasons in
// the gather buffers and (rand32: optional, the shard's rows of the caller's
// array) the verified rounds' randomness, straight from the device to the
// host as dgpu_recover_multi returns its signatures.  a's signature arrays
// are the staged device copies.
int shard_results_locked(dgpu_multi* m, int k, const verify_args& a, uint8_t* rand32) {
  if (a.n == 0) return DGPU_OK;
  dgpu_ctx* c = m->ctx[k];
  return results_out_locked(c, a, m->buf[k].bits.u8(), nullptr, m->buf[k].reasons.u8(), hipMemcpyDeviceToDevice, rand32,
                            c->stream);
}

inline int no_shard_done(int, const verify_args&) { return DGPU_OK; }

// The multi-device verify call over host records (dgpu_verify_multi,
// dgpu_verify_segment_multi, dgpu_check_rows_multi).  What varies per form
// comes as callables: src_of(k, lo, hi) is the message source of shard k =
// items [lo, hi) of the caller's arrays (a row form attaches the shard's
// rows_src); shard_done(k, args) runs on device k's thread once a non-empty
// shard's statuses are final (no_shard_done: nothing to add).  Everything else is the same for
// every form.  No verdict bitmap is gathered when verdict_bits is NULL, no reasons when reason
// is (the entry point decides whether either may be).
template <class SrcOf, class ShardDone>
int multi_verify(dgpu_multi* m, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint8_t* sigs,
                 size_t sig_stride, const uint32_t* sig_len, int mode, uint64_t rlc_seed, SrcOf&& src_of,
                 uint8_t* verdict_bits, uint8_t* reason, uint8_t* rand32, ShardDone&& shard_done) {
  if (!m) return set_err(DGPU_EINVAL, "null handle");
  if (n == 0) return DGPU_OK;
  std::lock_guard<std::mutex> mlk(m->mu);
  std::vector<std::unique_lock<std::mutex>> locks;
  for (dgpu_ctx* c : m->ctx) locks.emplace_back(c->mu);
  const int D = m->ndev;
  // per-device shard capacity (a multiple of 8 rounds; dgpu_shard_range's rule)
  const size_t per = (((n + (size_t)D - 1) / (size_t)D) + 7) & ~(size_t)7;
  std::vector<key_entry*> keys(D, nullptr);
  std::vector<verify_args> args(D);
  std::vector<size_t> lo(D);
  int rc;
  for (int k = 0; k < D; ++k) {
    dgpu_ctx* c = m->ctx[k];
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = get_key_locked(c, scheme, pk, pk_len, &keys[k]))) return rc;
    size_t hi;
    dgpu_shard_range(n, D, k, &lo[k], &hi);
    // RLC coefficients: an independent seed per device (positions restart at 0)
    args[k] = verify_args{scheme, hi - lo[k], src_of(k, lo[k], hi), sigs ? sigs + lo[k] * sig_stride : nullptr,
                          sig_stride, sig_len ? sig_len + lo[k] : nullptr, mode,
                          D > 1 ? splitmix_host(rlc_seed ^ (0x5EEDull * (uint64_t)(k + 1))) : rlc_seed};
    if ((rc = check_args(c, keys[k], args[k]))) return rc;
    multi_bufs& b = m->buf[k];
    // (the roots: sized for either group's)
    if ((rc = b.bits.ensure(per / 8)) || (rc = b.reasons.ensure(per)) || (rc = b.all_bits.ensure(D * per / 8)) ||
        (rc = b.all_reasons.ensure(D * per)) || (rc = b.root.ensure(layout_bytes<rlc_root_layout>(G2J_WORDS))) ||
        (rc = b.all_roots.ensure((size_t)D * layout_bytes<rlc_root_layout>(G2J_WORDS))))
      return rc;
    HIP_TRY(hipStreamWaitEvent(c->stream, c->done, 0));
  }
  const bool rlc = mode == DGPU_MODE_RLC;
  // the roots: rlc_root_layout (P, S: stride-1 Jacobian of the signature group)
  const size_t root_bytes = layout_bytes<rlc_root_layout>(sig_on_g1(scheme) ? G1J_WORDS : G2J_WORDS);
  // phase 1: stage the shard (the records of the device's shard through its
  // context's pinned ring, overlapped with the verification) and verify it
  // per round (or compute its RLC root)
  rc = for_each_device(m, [&](int k) -> int {
    dgpu_ctx* c = m->ctx[k];
    verify_args& a = args[k];
    hipStream_t s = c->stream;
    int r;
    if (a.n && (r = c->status.ensure(a.n))) return r;  // (a staging rehearsal packs it too: DGPU_TEST_STAGE_ONLY)
    if (rlc) {  // the shard's points and its root by bucket MSM (the leaves wait for a failing root)
      if (a.n) {
        c->rlc_pending = false;  // overwrites the points a pending per-rank root (dgpu_rlc_root_device) kept
        if ((r = stage_all_host_locked(c, a, s))) return r;
      }
      return rlc_shard_root_locked(c, a, m->buf[k].root.u8(), s);  // (ensured above)
    }
    if (a.n == 0) return DGPU_OK;
    // the shard's records through the context's pinned ring, slice by slice
    // beside the verification (verify_status_host_locked)
    if ((r = verify_status_host_locked(c, keys[k], a, s)) ||
        (r = shard_results_locked(m, k, a, rand32 ? rand32 + 32 * lo[k] : nullptr)))
      return r;
    return shard_done(k, a);
  });
  if (rc) return rc;
  if (rlc) {
    // the per-device roots to every device; one check of their sum on device 0
    std::vector<const void*> src(D);
    std::vector<void*> dst(D);
    for (int k = 0; k < D; ++k) {
      src[k] = m->buf[k].root.p;
      dst[k] = m->buf[k].all_roots.p;
    }
    if ((rc = multi_all_gather(m, src, dst, root_bytes))) return rc;
    dgpu_ctx* c0 = m->ctx[0];
    HIP_TRY(hipSetDevice(c0->device));
    bool fail = false;
    if ((rc = rlc_node_check_locked(c0, keys[0], (size_t)D, m->buf[0].all_roots.u8(), c0->stream, &fail)))
      return rc;
    rc = for_each_device(m, [&](int k) -> int {
      dgpu_ctx* c = m->ctx[k];
      const verify_args& a = args[k];
      if (a.n == 0) return DGPU_OK;
      int r;
      // (phase 1 left the shard's root in msm_root)
      if ((r = rlc_shard_finish_locked(c, keys[k], a, fail, (size_t)D, c->stream)) ||
          (r = shard_results_locked(m, k, a, rand32 ? rand32 + 32 * lo[k] : nullptr)))
        return r;
      return shard_done(k, a);
    });
    if (rc) return rc;
  }
  // the verdicts of every shard to every device (one grouped all-gather)
  for (int k = 0; k < D; ++k) {
    HIP_TRY(hipSetDevice(m->ctx[k]->device));
    if (args[k].n < per) {  // padding of a short (or empty) last shard
      const size_t b0 = (args[k].n + 7) / 8;
      HIP_TRY(hipMemsetAsync(m->buf[k].bits.u8() + b0, 0, per / 8 - b0, m->ctx[k]->stream));
    }
  }
  {
    std::vector<const void*> src(D), rsrc(D);
    std::vector<void*> dst(D), rdst(D);
    for (int k = 0; k < D; ++k) {
      src[k] = m->buf[k].bits.p;
      dst[k] = m->buf[k].all_bits.p;
      rsrc[k] = m->buf[k].reasons.p;
      rdst[k] = m->buf[k].all_reasons.p;
    }
    if (verdict_bits && (rc = multi_all_gather(m, src, dst, per / 8))) return rc;
    if (reason && (rc = multi_all_gather(m, rsrc, rdst, per))) return rc;
  }
  for (int k = 0; k < D; ++k) {
    HIP_TRY(hipSetDevice(m->ctx[k]->device));
    HIP_TRY(hipStreamSynchronize(m->ctx[k]->stream));
  }
  dgpu_ctx* c0 = m->ctx[0];
  HIP_TRY(hipSetDevice(c0->device));
  if (verdict_bits)
    HIP_TRY(hipMemcpyAsync(verdict_bits, m->buf[0].all_bits.p, (n + 7) / 8, hipMemcpyDeviceToHost, c0->stream));
  if (reason) HIP_TRY(hipMemcpyAsync(reason, m->buf[0].all_reasons.p, n, hipMemcpyDeviceToHost, c0->stream));
  for (int k = 0; k < D; ++k) {
    HIP_TRY(hipSetDevice(m->ctx[k]->device));
    HIP_TRY(hipEventRecord(m->ctx[k]->done, m->ctx[k]->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx[k]->stream));
  }
  return DGPU_OK;
}

}  // namespace

extern "C" {

int dgpu_verify_multi(dgpu_multi* m, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint64_t* rounds,
                      const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len, const uint8_t* prev,
                      size_t prev_stride, const uint32_t* prev_len, int mode, uint64_t rlc_seed,
                      uint8_t* verdict_bits, uint8_t* reason) {
  if (m && n && !verdict_bits) return set_err(DGPU_EINVAL, "null verdict buffer");
  const bool chained = scheme == DGPU_SCHEME_CHAINED;
  return multi_verify(
      m, scheme, pk, pk_len, n, sigs, sig_stride, sig_len, mode, rlc_seed,
      [&](int, size_t lo, size_t) {
        return beacon_src(rounds + lo, chained ? prev + lo * prev_stride : nullptr, prev_stride,
                          chained ? prev_len + lo : nullptr, chained);
      },
      verdict_bits, reason, nullptr, no_shard_done);
}

// The linked form over the node: shard 0 is dgpu_verify_segment's source (the
// caller's seed by value), shard k > 0 the halo form with record lo_k - 1 of
// the caller's arrays as its halo, staged ahead of the shard's own records
// (host_stager::stage_slice).
int dgpu_verify_segment_multi(dgpu_multi* m, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_round,
                              size_t n, const uint8_t* sigs, size_t sig_stride, const uint32_t* sig_len,
                              const uint8_t* seed_prev, size_t seed_prev_len, int mode, uint64_t rlc_seed,
                              uint8_t* verdict_bits, uint8_t* reason, uint8_t* randomness32) {
  int rc = check_segment_args(scheme, first_round, n, seed_prev, seed_prev_len);
  if (rc) return rc;
  const bool chained = scheme == DGPU_SCHEME_CHAINED;
  if (n && (!sigs || !sig_len)) return set_err(DGPU_EINVAL, "bad signature buffers");
  if (m && n && !verdict_bits) return set_err(DGPU_EINVAL, "null verdict buffer");
  return multi_verify(
      m, scheme, pk, pk_len, n, sigs, sig_stride, sig_len, mode, rlc_seed,
      [&](int, size_t lo, size_t hi) {
        const uint8_t* s_lo = sigs + lo * sig_stride;
        if (lo == 0 || lo == hi)  // (an empty shard runs nothing: any source)
          return linked_src(first_round, s_lo, sig_stride, sig_len + lo, seed_prev, seed_prev_len, chained);
        return halo_src(first_round + lo, s_lo, sig_stride, sig_len + lo, s_lo - sig_stride, sig_len + lo - 1, chained);
      },
      verdict_bits, reason, randomness32, no_shard_done);
}

// dgpu_check_rows over the node.  The rows shard like every batch here; the
// visited positions follow the rows: shard 0 owns them from 0, a later
// non-empty shard k from its first key, the last non-empty shard up to count
// -- so a run of missing rounds in front of a shard's first key belongs to the
// shard before it -- and each device builds the list of its own positions.
// The host concatenates the lists in shard order; no collective carries them.
int dgpu_check_rows_multi(dgpu_multi* m, int scheme, const uint8_t* pk, size_t pk_len, size_t n, const uint8_t* base,
                          const uint64_t* row_off, const uint32_t* row_len, const uint64_t* keys, size_t sig_stride,
                          size_t prev_stride, int mode, uint64_t rlc_seed, uint64_t first, size_t count,
                          uint64_t* faulty_pos, uint64_t* faulty_val, size_t faulty_cap, uint64_t* n_faulty,
                          uint64_t* left_rows, size_t left_cap, uint64_t* n_left, uint8_t* reason) {
  if (!m) return set_err(DGPU_EINVAL, "null handle");
  if (n == 0) {  // shard 0 owns every position
    std::lock_guard<std::mutex> mlk(m->mu);
    return dgpu_check_rows(m->ctx[0], scheme, pk, pk_len, 0, base, row_off, row_len, keys, sig_stride, prev_stride, mode,
                           rlc_seed, first, count, faulty_pos, faulty_val, faulty_cap, n_faulty, left_rows, left_cap,
                           n_left, reason);
  }
  int rc = check_rows_args(n, base, row_off, row_len, keys, first, count, faulty_pos, faulty_val, faulty_cap, n_faulty,
                           left_rows, left_cap, n_left);
  if (rc) return rc;
  const int D = m->ndev;
  // each device's rows_src over its shard, the positions [p0[k], p0[k] + pcount[k])
  // of the visited range device k owns, and the lists each device returns
  // (positions relative to p0[k], rows to the shard)
  std::vector<rows_src> R(D);
  std::vector<uint64_t> p0(D, 0);
  std::vector<size_t> pcount(D, 0);
  std::vector<check_lists> lists(D);
  std::vector<size_t> lo(D), hi(D);
  for (int k = 0; k < D; ++k) dgpu_shard_range(n, D, k, &lo[k], &hi[k]);
  for (int k = 0; k < D; ++k) {
    if (lo[k] == hi[k]) continue;  // (the non-empty shards are the first ones)
    p0[k] = k ? keys[lo[k]] - first : 0;
    const bool last = k + 1 == D || lo[k + 1] == hi[k + 1];
    pcount[k] = (size_t)((last ? (uint64_t)count : keys[lo[k + 1]] - first) - p0[k]);
  }
  const bool chained = scheme == DGPU_SCHEME_CHAINED;
  // No verdict bitmap: the lists are the result.  shard_done: the faulty list of the positions
  // device k owns, once its shard's statuses are final (synchronises the device's stream).
  rc = multi_verify(
      m, scheme, pk, pk_len, n, nullptr, sig_stride, nullptr, mode, rlc_seed,
      [&](int k, size_t lo_k, size_t) {
        R[k] = rows_src_of(base, row_off + lo_k, row_len + lo_k, keys + lo_k, sig_stride, prev_stride);
        return rows_records_src(&R[k], prev_stride, chained);
      },
      nullptr, reason, nullptr,
      [&](int k, const verify_args& a) {
        dgpu_ctx* c = m->ctx[k];
        return check_lists_locked(c, first + p0[k], pcount[k], a.n, a.m.rows->d_keys, faulty_cap, left_cap,
                                  lists[k], c->stream);
      });
  if (rc) return rc;
  check_lists all;
  for (int k = 0; k < D; ++k) {
    const check_lists& L = lists[k];
    all.n_faulty += L.n_faulty, all.n_left += L.n_left;
    for (size_t i = 0; i < L.pos.size(); ++i) all.pos.push_back(L.pos[i] + p0[k]), all.val.push_back(L.val[i]);
    for (uint64_t r : L.left) all.left.push_back(r + lo[k]);
  }
  check_lists_store(all, faulty_pos, faulty_val, faulty_cap, n_faulty, left_rows, left_cap, n_left);
  return DGPU_OK;
}

}  // extern "C"

extern "C" {

int dgpu_multi_set_group_scheme(dgpu_multi* m, int scheme, int t, int n, const uint8_t* commits, size_t commit_len) {
  if (!m) return set_err(DGPU_EINVAL, "null handle");
  std::lock_guard<std::mutex> mlk(m->mu);
  for (int k = 0; k < m->ndev; ++k) {
    int rc = dgpu_set_group_scheme(m->ctx[k], scheme, t, n, commits, commit_len);
    if (rc) return set_err(rc, "device %d: %s", m->devs[k], std::string(g_last_error).c_str());
  }
  return DGPU_OK;
}

int dgpu_multi_set_group_wide(dgpu_multi* m, int scheme, int t, int n, const uint8_t* commits, size_t commit_len) {
  if (!m) return set_err(DGPU_EINVAL, "null handle");
  std::lock_guard<std::mutex> mlk(m->mu);
  for (int k = 0; k < m->ndev; ++k) {
    int rc = dgpu_set_group_wide(m->ctx[k], scheme, t, n, commits, commit_len);
    if (rc) return set_err(rc, "device %d: %s", m->devs[k], std::string(g_last_error).c_str());
  }
  return DGPU_OK;
}

int dgpu_multi_set_group(dgpu_multi* m, int t, int n, const uint8_t* commits48) {
  if (!m) return set_err(DGPU_EINVAL, "null handle");
  std::lock_guard<std::mutex> mlk(m->mu);
  for (int k = 0; k < m->ndev; ++k) {
    int rc = dgpu_set_group(m->ctx[k], t, n, commits48);
    if (rc) return set_err(rc, "device %d: %s", m->devs[k], std::string(g_last_error).c_str());
  }
  return DGPU_OK;
}

// Threshold recovery over the node: rounds shard contiguously like the verify
// batch (dgpu_shard_range); each device stages and recovers its shard
// (recover_device_locked: VerifyPartial / selection / Lagrange + MSM /
// VerifyRecovered), the per-device recovery bitmaps are all-gathered (RCCL),
// and the recovered signatures and per-partial statuses -- data, not
// verdicts -- go to the host straight from the device that made them.
int dgpu_recover_multi(dgpu_multi* m, size_t n_rounds, const uint8_t* msgs32, size_t m_slots, const uint8_t* partials,
                       size_t partial_stride, const uint32_t* partial_len, uint8_t* out_sigs, uint8_t* ok_bits,
                       uint8_t* partial_valid) {
  if (!m) return set_err(DGPU_EINVAL, "null multi handle");
  if (n_rounds == 0) return DGPU_OK;  // an empty batch: no-op, NULL buffers accepted
  if (!msgs32 || !partials || !partial_len || !out_sigs || !ok_bits) return set_err(DGPU_EINVAL, "null argument");
  if (m_slots == 0) return set_err(DGPU_EINVAL, "need m >= 1 partial slots");
  const size_t items = n_rounds * m_slots;
  for (size_t i = 0; i < items; ++i)
    if (partial_len[i] > partial_stride) return set_err(DGPU_EINVAL, "partial_len[%zu] > stride", i);
  std::lock_guard<std::mutex> mlk(m->mu);
  std::vector<std::unique_lock<std::mutex>> locks;
  for (dgpu_ctx* c : m->ctx) locks.emplace_back(c->mu);
  const int D = m->ndev;
  const size_t per = (((n_rounds + (size_t)D - 1) / (size_t)D) + 7) & ~(size_t)7;
  std::vector<size_t> lo(D), hi(D);
  int rc;
  for (int k = 0; k < D; ++k) {
    dgpu_ctx* c = m->ctx[k];
    if (!c->grp_t) return set_err(DGPU_ENOKEY, "device %d: no threshold group installed (dgpu_multi_set_group)",
                                  m->devs[k]);
    if (partial_stride < group_partial_bytes(c))
      return set_err(DGPU_EINVAL, "need stride >= %zu", group_partial_bytes(c));
    dgpu_shard_range(n_rounds, D, k, &lo[k], &hi[k]);
    HIP_TRY(hipSetDevice(c->device));
    multi_bufs& b = m->buf[k];
    if ((rc = b.bits.ensure(per / 8)) || (rc = b.all_bits.ensure(D * per / 8))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->stream, c->done, 0));
  }
  std::vector<std::vector<uint8_t>> stv(D);
  rc = for_each_device(m, [&](int k) -> int {
    dgpu_ctx* c = m->ctx[k];
    hipStream_t s = c->stream;
    const size_t nr = hi[k] - lo[k], it = nr * m_slots;
    int r;
    if (nr == 0) {
      HIP_TRY(hipMemsetAsync(m->buf[k].bits.p, 0, per / 8, s));
      return DGPU_OK;
    }
    if ((r = c->rec_msgs.ensure(nr * 32)) || (r = c->rec_parts.ensure(it * partial_stride)) ||
        (r = c->rec_plen.ensure(it * 4)) || (r = c->rec_out.ensure(nr * 96)) || (r = c->rec_ok.ensure(nr)) ||
        (r = c->out_reason.ensure(it)))
      return r;
    HIP_TRY(hipMemcpyAsync(c->rec_msgs.p, msgs32 + lo[k] * 32, nr * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_parts.p, partials + lo[k] * m_slots * partial_stride, it * partial_stride,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_plen.p, partial_len + lo[k] * m_slots, it * 4, hipMemcpyHostToDevice, s));
    if ((r = recover_device_locked(c, nr, c->rec_msgs.u8(), m_slots, c->rec_parts.u8(), partial_stride, c->rec_plen.u32(),
                                   c->rec_out.u8(), c->rec_ok.u8(), partial_valid ? c->out_reason.u8() : nullptr, s)))
      return r;
    HIP_TRY(hipMemsetAsync(m->buf[k].bits.p, 0, per / 8, s));
    RC_TRY(launch_n(k_pack_ok, (nr + 7) / 8, 256, s, nr, c->rec_ok.u8(), m->buf[k].bits.u8()));
    const size_t sb = group_sig_bytes(c);  // 48 for a G1-signature group
    HIP_TRY(hipMemcpyAsync(out_sigs + lo[k] * sb, c->rec_out.p, nr * sb, hipMemcpyDeviceToHost, s));
    if (partial_valid) {
      stv[k].resize(it);
      HIP_TRY(hipMemcpyAsync(stv[k].data(), c->out_reason.p, it, hipMemcpyDeviceToHost, s));
    }
    return DGPU_OK;
  });
  if (rc) return rc;
  std::vector<const void*> src(D);
  std::vector<void*> dst(D);
  for (int k = 0; k < D; ++k) {
    src[k] = m->buf[k].bits.p;
    dst[k] = m->buf[k].all_bits.p;
  }
  if ((rc = multi_all_gather(m, src, dst, per / 8))) return rc;
  dgpu_ctx* c0 = m->ctx[0];
  HIP_TRY(hipSetDevice(c0->device));
  HIP_TRY(hipMemcpyAsync(ok_bits, m->buf[0].all_bits.p, (n_rounds + 7) / 8, hipMemcpyDeviceToHost, c0->stream));
  for (int k = 0; k < D; ++k) {
    HIP_TRY(hipSetDevice(m->ctx[k]->device));
    HIP_TRY(hipEventRecord(m->ctx[k]->done, m->ctx[k]->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx[k]->stream));
  }
  if (partial_valid)
    for (int k = 0; k < D; ++k)
      for (size_t i = 0; i < stv[k].size(); ++i) partial_valid[lo[k] * m_slots + i] = stv[k][i] == ST_OK;
  return DGPU_OK;
}

}  // extern "C"
