/*
 * drand_gpu.h -- C ABI of the MI355X batch beacon verifier (libdrand_gpu.so).
 *
 * Drop-in boundary for drand's verification path.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo):
 *
 *   chain.NewVerifier / Verifier.VerifyBeacon    chain/verify.go:18-20, 38-45
 *   Verifier.DigestMessage + RoundToBytes        chain/verify.go:24-32, chain/store.go:42-46
 *   key.Scheme.VerifyRecovered (bls.Verify (R))  chain/verify.go:44, key/curve.go:36
 *   kyber G2 Hash (kilic HashToCurve (R))        key/curve.go:36 (pinned by key/curve_test.go:10-30)
 *   KeyGroup.Point().UnmarshalBinary (pk)        chain/convert.go:19-38 (InfoFromProto)
 *   scheme IDs                                   common/scheme/scheme.go:9-20
 *
 * Callers it serves (all only test err != nil, so one verdict bit per round
 * carries the full reference contract): chain/beacon/sync_manager.go:212
 * (CheckPastBeacons), :397 (tryNode), client/verify.go:162,201,
 * lp2p/client/validator.go:66.
 *
 * Conventions
 *  - Plain pointers and sizes only; all host buffers are caller-owned and are
 *    not retained after a call returns (cgo-safe).
 *  - Return codes: DGPU_OK (0) or a negative DGPU_E* value; the message is in
 *    dgpu_last_error() (thread-local: the calling thread's last failure; a
 *    successful dgpu_open clears it).
 *  - A context is bound to one GPU and serializes its own calls internally;
 *    any thread may call.  Calls on one context are also ordered on the
 *    device: each call's work starts after the previous call's, whatever
 *    streams the *_device entry points are given.  There is no CPU fallback:
 *    without a usable GPU, dgpu_open fails with DGPU_EDEVICE.
 *  - Streams (*_device entry points): `stream` is a hipStream_t of the
 *    context's device and the call's work is enqueued on it, ordered after
 *    everything the caller enqueued on it before the call (zero-fills, input
 *    copies) and before anything enqueued after it (readouts, collectives).
 *    NULL is the device's legacy default (null) stream -- torch's default
 *    stream -- exactly as in HIP itself.  A caller that does not bind HIP
 *    (cgo) waits for results with dgpu_synchronize.
 *  - Public keys are passed per call (dgpu_verify_beacons*, like
 *    VerifyBeacon(b, pubkey), chain/verify.go:38) and cached decoded per
 *    context (8 keys, LRU), so one context serves any number of chains and
 *    schemes; dgpu_set_pubkey + dgpu_verify_batch* keep the ABI-1 form.
 *  - Verdict bitmaps: bit (i % 8) of byte (i / 8) is 1 iff round i verifies,
 *    i.e. iff the reference's VerifyBeacon returns nil.
 */
#ifndef DRAND_GPU_H
#define DRAND_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): a NULL stream in the *_device entry points is the device's
 * legacy default (null) stream, no longer the context's own stream;
 * dgpu_synchronize added; dgpu_stage_times returns the count of stages the
 * call recorded (may exceed max_stages); RLC mode accepted for the G1-signature
 * schemes; DGPU_MAX_STAGES 32.
 * Added to ABI 3 without a version change (additive only): threshold
 * recovery for the G1-signature schemes -- dgpu_set_group_scheme,
 * dgpu_multi_set_group_scheme, dgpu_make_partials_scheme; the recover entry
 * points follow the installed group's scheme (their out_sigs96 parameters
 * are now out_sigs, stride 96 or 48 bytes per round).  Also additive:
 * dgpu_verify_segment and dgpu_verify_segment_device, a linked chain segment
 * verified from its signatures alone, with the rounds' randomness.  Also
 * additive: linked segments across GPUs -- dgpu_verify_segment_shard_device
 * (one shard, its first item's previous signature a one-record halo in device
 * memory), dgpu_rlc_root_segment_device (step 1 of the per-rank RLC protocol
 * over such a shard) and dgpu_verify_segment_multi.  Also additive: stored rows
 * (dgpu_decode_rows_device, dgpu_verify_rows) and the check-chain loop's
 * faulty list built on the device (dgpu_faulty_rounds_device, dgpu_check_rows,
 * dgpu_check_rows_multi).  Also additive: verification under a key per record
 * (dgpu_verify_keyed, dgpu_verify_keyed_device, reason DGPU_REASON_KEY) and
 * VerifyPartial of every slot without a recovery (dgpu_verify_partials,
 * dgpu_verify_partials_device).  Also additive: threshold groups above t = 32
 * (dgpu_set_group_wide, dgpu_multi_set_group_wide, DGPU_MAX_THRESHOLD). */
#define DGPU_ABI_VERSION 3

/* scheme IDs (common/scheme/scheme.go:9,12; bls-unchained-on-g1 added by this build) */
enum {
  DGPU_SCHEME_CHAINED = 0,      /* "pedersen-bls-chained":   msg = SHA256(prev || BE64(round)) */
  DGPU_SCHEME_UNCHAINED = 1,    /* "pedersen-bls-unchained": msg = SHA256(BE64(round))        */
  DGPU_SCHEME_UNCHAINED_G1 = 2, /* "bls-unchained-on-g1":    G1 signatures (48 B), G2 public key
                                   (96 B); msg = SHA256(BE64(round)) hashed to G1 under the G2
                                   suite's DST (upstream drand's choice (R), unpinned here)  */
  DGPU_SCHEME_G1_RFC9380 = 3    /* "bls-unchained-g1-rfc9380": as above, RFC 9380 G1 DST    */
};

enum {
  DGPU_OK = 0,
  DGPU_EINVAL = -1,
  DGPU_EDEVICE = -2,
  DGPU_ENOMEM = -3,
  DGPU_EUNSUPPORTED = -4,
  DGPU_ENOKEY = -5
};

/* per-round reason codes (optional output of the verify calls) */
enum {
  DGPU_REASON_OK = 0,
  DGPU_REASON_DECODE = 1,   /* kyber UnmarshalBinary error: length, flags, x >= p, not on curve */
  DGPU_REASON_SUBGROUP = 2, /* UnmarshalBinary error: not in the r-order subgroup              */
  DGPU_REASON_PAIRING = 3,  /* bls: invalid signature                                          */
  DGPU_REASON_INFINITY = 4, /* signature decodes to the identity: pairing check fails          */
  DGPU_REASON_KEY = 5       /* the record's key (dgpu_verify_keyed): undecodable, not in the
                               subgroup, the identity, or (device form) an index outside the table */
};

enum { DGPU_MODE_PER_ROUND = 0, DGPU_MODE_RLC = 1 };

/* Empty batches: every batch entry point (verify, verify_recovered, recover,
 * their _device and _multi forms) returns DGPU_OK for n = 0 rounds without
 * reading or writing any buffer, and accepts NULL record / output pointers
 * then (tests/test_gpu_boundary.py::test_empty_batches_are_no_ops). */

typedef struct dgpu_ctx dgpu_ctx;

int dgpu_abi_version(void);
const char *dgpu_last_error(void);

/* Open device `device` (HIP ordinal).  Replaces nothing in the reference: the
 * Go side would hold one context per GPU inside crypto/gpu.BatchVerifier.
 * The environment is read once here, and only these shipped thresholds and
 * kernel-family switches (verdicts are identical under every setting):
 *   DGPU_THR_MIN=<items> (default 65536): pairing batches (per-round chunks
 *     and RLC node checks) on fewer items take the 12- / 8-lane engine
 *     kernels, which fill the chip and cut the per-item latency at small sizes;
 *   DGPU_RLC_MIN=<rounds> (default 131072): DGPU_MODE_RLC batches of fewer
 *     rounds run the per-round path (below that size the combination's fixed
 *     costs make it the slower one);
 *   DGPU_COF_ENGINE_MAX=<rounds>, DGPU_FE_GS_MAX=<items> (default 16384
 *     each): the small-call latency path (hash cofactor on the engine ladder,
 *     Granger-Scott final exponentiation); 0 turns it off;
 *   DGPU_ENG_CHUNK=<rounds>: engine chunk size (default: 1Mi, or what half
 *     the free HBM holds);
 *   DGPU_LANES=1: the whole call on one stream (default: two streams over
 *     the halves of a large per-round G2 batch, the decode beside the hash);
 *   DGPU_LINES=engine, DGPU_KB_CHAIN=lanes: the Miller loops' T-steps / the
 *     final exponentiation's compressed chains on the 12- / 8-lane engine at
 *     every size; DGPU_FE=gs: the Granger-Scott final exponentiation.
 * Variants measured and not shipped, and test hooks, are read only by the
 * A/B build of the same sources (-DDG_AB_KNOBS, drand_amd/libdrand_gpu_ab.so). */
int dgpu_open(int device, dgpu_ctx **out);
void dgpu_close(dgpu_ctx *ctx);

/* Scheme name -> id, "" -> default chained (scheme.GetSchemeByIDWithDefault,
 * common/scheme/scheme.go:37-48).  Returns the id or DGPU_EINVAL. */
int dgpu_scheme_from_name(const char *name);

/* Decode and install the group public key (chain.Info.PublicKey,
 * chain/convert.go:20-23): 48-byte compressed G1 for the G2-signature
 * schemes, 96-byte compressed G2 for the G1-signature schemes (which also
 * precomputes the key's fixed Miller-loop lines).  Rejects malformed or
 * out-of-subgroup keys (DGPU_EINVAL). */
int dgpu_set_pubkey(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t len);

/* Contiguous shard [lo, hi) of item k among ndev devices as dgpu_verify_multi
 * splits a batch of n: shards are multiples of 8 items (whole verdict-bitmap
 * bytes) and the last takes the remainder.  Host-only bookkeeping. */
void dgpu_shard_range(size_t n, int ndev, int k, size_t *lo, size_t *hi);

/* Batch form of Verifier.VerifyBeacon(b, pubkey) (chain/verify.go:38-45), the
 * public key passed per call (48-byte compressed G1, or 96-byte compressed G2
 * for the G1-signature schemes; decoded, subgroup-checked and cached by the
 * context; DGPU_EINVAL if rejected).  Records as dgpu_verify_batch. */
int dgpu_verify_beacons(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n,
                        const uint64_t *rounds, const uint8_t *sigs, size_t sig_stride, const uint32_t *sig_len,
                        const uint8_t *prev, size_t prev_stride, const uint32_t *prev_len, int mode,
                        uint64_t rlc_seed, uint8_t *verdict_bits, uint8_t *reason);

/* dgpu_verify_beacons over device-resident records (as dgpu_verify_batch_device):
 * a record with prev_len[i] > prev_stride is not read past its stride and
 * fails with reason DGPU_REASON_DECODE. */
int dgpu_verify_beacons_device(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n,
                               const uint64_t *d_rounds, const uint8_t *d_sigs, size_t sig_stride,
                               const uint32_t *d_sig_len, const uint8_t *d_prev, size_t prev_stride,
                               const uint32_t *d_prev_len, int mode, uint64_t rlc_seed, uint8_t *d_verdict_bits,
                               uint8_t *d_reason, void *stream);

/* Stored beacon rows -> fixed-stride records, on the device (check-chain
 * ingest: the rows of the bolt beacon store as Beacon.Marshal wrote them,
 * chain/beacon.go:34-37).  Row i is d_row_len[i] bytes at d_rows +
 * d_row_off[i] inside the device buffer [d_rows, d_rows + rows_bytes); nothing
 * outside that buffer is read, whatever its alignment, and a row whose range
 * leaves it is not read and gets ok = 0.  The contract is the host decoder's
 * (dgpu_ingest_decode of include/drand_ingest.h), byte for byte.  Canonical
 * form only:
 *   {"PreviousSig":<hex or null>,"Round":<uint64>,"Signature":<hex or null>}
 * in Go's field order with no whitespace; a field is null or a quoted
 * even-length hex string of either letter case holding at most its stride in
 * bytes; Round is 1-20 digits with no leading zero that fit 64 bits; the
 * closing brace is the row's last byte.  A canonical row: d_ok[i] = 1,
 * d_rounds[i], d_sig_len[i] bytes at d_sigs + i*sig_stride and d_prev_len[i]
 * bytes at d_prev + i*prev_stride, each zero-padded to its stride.  Any other
 * row: d_ok[i] = 0, round 0, both lengths 0, both records zeroed -- an
 * ordinary decode failure for the verify calls; the caller passes such rows
 * to its full hexjson decoder.  No field is written past its stride.  The
 * outputs must not overlap the rows or each other.  Asynchronous on `stream`
 * (as dgpu_verify_beacons_device); n = 0 is a no-op that accepts NULL
 * pointers. */
int dgpu_decode_rows_device(dgpu_ctx *ctx, size_t n, const uint8_t *d_rows, size_t rows_bytes,
                            const uint64_t *d_row_off, const uint32_t *d_row_len, uint64_t *d_rounds, uint8_t *d_sigs,
                            size_t sig_stride, uint32_t *d_sig_len, uint8_t *d_prev, size_t prev_stride,
                            uint32_t *d_prev_len, uint8_t *d_ok, void *stream);

/* dgpu_verify_beacons over stored rows in host memory: row i is row_len[i]
 * bytes at base + row_off[i], exactly what dgpu_ingest_scan emits over the
 * mapped store.  The rows are decoded on the device: row_ok (n bytes) and
 * rounds_out (optional, n values) equal the host decoder's ok and rounds at
 * these strides, and verdict_bits and reason equal dgpu_verify_beacons on the
 * arrays the host decoder writes, under the same key, mode and rlc_seed (a
 * row with row_ok = 0 is a zeroed record: reason DGPU_REASON_DECODE; the
 * caller passes it to its full hexjson decoder).  A row longer than any
 * canonical row at the strides, 64 + 2 (sig_stride + prev_stride) bytes, is
 * not canonical and is not staged.  The rows go through the pinned ring of
 * dgpu_staging_stats packed back to back, cut by bytes into pieces of whole
 * rows (a piece is the longest run of rows whose packed bytes, rounded up to
 * 8, plus 12 bytes per row fit a 16 MiB slot); each piece is decoded on the
 * copy stream behind its DMA, and a slice's hash waits for that slice's
 * decode alone.  Staged bytes (dgpu_staging_stats):
 *   sum of row_len[i] over the rows within 64 + 2 (sig_stride + prev_stride)
 *   + 12 n   (each row's position and length). */
int dgpu_verify_rows(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n, const uint8_t *base,
                     const uint64_t *row_off, const uint32_t *row_len, size_t sig_stride, size_t prev_stride, int mode,
                     uint64_t rlc_seed, uint64_t *rounds_out, uint8_t *row_ok, uint8_t *verdict_bits, uint8_t *reason);

/* The faulty list of SyncManager.CheckPastBeacons (chain/beacon/
 * sync_manager.go:188-222) over one window, built on the device from the
 * outputs of the row verification.  The loop visits rounds first + j for j in
 * [0, count) (first + count must not overflow 64 bits: DGPU_EINVAL).  The
 * window's n rows carry d_keys[r] (the bolt key: the round the loop's Get asks
 * for, as dgpu_ingest_scan emits it), d_row_ok[r] and d_rounds[r] (the
 * decoder's outputs, dgpu_decode_rows_device) and d_reason[r] (the row's
 * DGPU_REASON_* code, 0 = valid).  Position j (one rule, check_rows_outcome of
 * drand_amd/csrc/check_rows.cuh):
 *   no row has d_keys[r] == first + j       faulty, value first + j (:202-210)
 *   the row exists, d_row_ok[r] == 0        left: r is listed in d_left_rows
 *                                           for the caller's full hexjson
 *                                           decoder; nothing in the faulty list
 *   the row exists and is ok, reason != 0   faulty, value d_rounds[r] (:212-214:
 *                                           the stored Round, not the key)
 *   otherwise                               nothing
 * A row whose key lies outside [first, first + count) takes no part.
 * d_faulty_pos[i] / d_faulty_val[i]: position j and value of the i-th faulty
 * entry, in ascending position -- the reference's ascending walk; d_left_rows:
 * the left rows in ascending row index.  The compaction is ordered (flags, a
 * prefix sum, a scatter): no atomic append, no sort.  d_counts[0], d_counts[1]:
 * the totals of faulty entries and of left rows, which may exceed the caps;
 * entries at or beyond a cap are not written and nothing is written past
 * either buffer.  d_keys must be strictly ascending; with duplicate keys which
 * row a position takes is unspecified, but no access leaves the given buffers
 * whatever the keys hold.  n = 0 with count > 0 makes every position faulty;
 * count = 0 is a no-op that accepts NULL pointers (d_counts is not written).
 * n < 2^32 - 1.  The scratch (position map, flags, block sums: 5 count + 16
 * ceil(count / 256) bytes) is the context's.  Asynchronous on `stream` (as
 * dgpu_verify_beacons_device). */
int dgpu_faulty_rounds_device(dgpu_ctx *ctx, uint64_t first, size_t count, size_t n, const uint64_t *d_keys,
                              const uint8_t *d_row_ok, const uint64_t *d_rounds, const uint8_t *d_reason,
                              uint64_t *d_faulty_pos, uint64_t *d_faulty_val, size_t faulty_cap,
                              uint64_t *d_left_rows, size_t left_cap, uint64_t *d_counts, void *stream);

/* CheckPastBeacons over one window of stored rows in one call: the rows,
 * key, strides, mode and seed of dgpu_verify_rows, the rows' keys (n values,
 * as dgpu_ingest_scan emits them) and the visited range.  Synchronous.  The
 * rows are decoded and verified exactly as dgpu_verify_rows does, then
 * dgpu_faulty_rounds_device runs behind that on the same stream over the
 * decoder's ok flags and rounds and the final statuses.  Contract: faulty_pos,
 * faulty_val and left_rows (entries below their caps) and *n_faulty, *n_left
 * (the totals) equal that rule applied to dgpu_verify_rows' row_ok,
 * rounds_out and reason for the same rows, key, mode and rlc_seed.  The caller
 * passes each left row to its full hexjson decoder (position keys[r] - first:
 * an undecodable row faults its own round, a decodable one is verified and a
 * failure faults its stored Round) and merges by position.  Only the two
 * lists and their totals are copied back -- 16 bytes, then 16 bytes per
 * faulty entry and 8 per left row below the caps -- and reason (optional, n
 * bytes, as dgpu_verify_rows writes it) only when given.  DGPU_EINVAL before
 * any device work: keys not strictly ascending, a key outside [first, first +
 * count), first + count overflowing 64 bits, a NULL buffer with a nonzero
 * size (rows and keys with n > 0, a list with a nonzero cap, n_faulty,
 * n_left).  n = 0 verifies nothing (the key and scheme are still checked) and
 * makes every position faulty; count = 0 (hence n = 0) writes two zero
 * totals.  The keys are staged beside the rows through the same ring, slice
 * by slice.  Staged bytes (dgpu_staging_stats):
 *   dgpu_verify_rows' bytes + 8 n   (each row's key). */
int dgpu_check_rows(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n, const uint8_t *base,
                    const uint64_t *row_off, const uint32_t *row_len, const uint64_t *keys, size_t sig_stride,
                    size_t prev_stride, int mode, uint64_t rlc_seed, uint64_t first, size_t count,
                    uint64_t *faulty_pos, uint64_t *faulty_val, size_t faulty_cap, uint64_t *n_faulty,
                    uint64_t *left_rows, size_t left_cap, uint64_t *n_left, uint8_t *reason);

/* A linked chain segment verified from its signatures alone: the walk from a
 * point of trust, client/verify.go:118-178, which builds each beacon as
 * {PreviousSig: the signature before it, Round, Signature} and (line 207)
 * takes the verified round's randomness, chain/beacon.go:51-54
 * RandomnessFromSignature = SHA-256(signature).  The caller passes the first
 * round, the n signatures (records as dgpu_verify_beacons: sig_len[i] bytes
 * at sigs + i*sig_stride) and one seed "previous signature" (host pointer,
 * seed_prev_len <= 96 bytes, else DGPU_EINVAL; may be NULL with length 0; it
 * is copied before the call returns, in the _device form too); round numbers
 * and previous signatures are derived on the device.  Verdict bits and
 * reasons equal dgpu_verify_beacons_device on the records
 *   rounds[i] = first_round + i          (first_round + n - 1 must not
 *                                         overflow 64 bits: DGPU_EINVAL)
 *   prev[0] = seed_prev, prev_len[0] = seed_prev_len
 *   prev[i] = sigs[i-1], prev_len[i] = sig_len[i-1], prev_stride = sig_stride
 * under the same key, mode and rlc_seed, so the first zero bit is where the
 * reference's walk returns "verifying beacon".  A sig_len[i] above sig_stride
 * is a decode failure of round i and (chained scheme) of round i + 1, never
 * an argument error, in both forms.  The unchained and G1-signature schemes
 * ignore previous signatures: only the implicit round numbers apply.
 * randomness32 (optional, n x 32 bytes): SHA-256 of round i's signature where
 * round i verifies, 32 zero bytes where it does not.
 * The host form stages each signature once -- n x (sig_stride + 4) bytes
 * (dgpu_staging_stats), where the explicit records of a chained scheme take
 * n x (2 sig_stride + 16) -- and returns the randomness with the verdicts. */
int dgpu_verify_segment(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, uint64_t first_round, size_t n,
                        const uint8_t *sigs, size_t sig_stride, const uint32_t *sig_len, const uint8_t *seed_prev,
                        size_t seed_prev_len, int mode, uint64_t rlc_seed, uint8_t *verdict_bits, uint8_t *reason,
                        uint8_t *randomness32);

/* dgpu_verify_segment over device-resident signatures, asynchronous on
 * `stream` (as dgpu_verify_beacons_device); seed_prev is a host pointer, like
 * pk, and may be freed on return. */
int dgpu_verify_segment_device(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, uint64_t first_round,
                               size_t n, const uint8_t *d_sigs, size_t sig_stride, const uint32_t *d_sig_len,
                               const uint8_t *seed_prev, size_t seed_prev_len, int mode, uint64_t rlc_seed,
                               uint8_t *d_verdict_bits, uint8_t *d_reason, uint8_t *d_randomness32, void *stream);

/* One shard of a linked segment, device-resident, asynchronous on `stream`:
 * as dgpu_verify_segment_device with the seed replaced by a device halo.
 * first_round is the shard's own first round; the previous signature of its
 * first item is the one-record halo in device memory -- the neighbouring
 * shard's last record, wherever a copy or a collective put it: *d_halo_len
 * bytes at d_halo, a record of stride sig_stride like the shard's own (not
 * capped at 96 bytes; never read past the stride).  Verdict bits, reasons and
 * randomness equal dgpu_verify_beacons_device on the records
 *   rounds[i] = first_round + i          (first_round + n - 1 must not
 *                                         overflow 64 bits: DGPU_EINVAL)
 *   prev[0] = halo, prev_len[0] = *d_halo_len
 *   prev[i] = sigs[i-1], prev_len[i] = sig_len[i-1], prev_stride = sig_stride
 * under the same key, mode and rlc_seed (randomness as dgpu_verify_segment
 * defines it), so *d_halo_len > sig_stride is a decode failure of the first
 * item, exactly what an over-long record does to the item after it inside a
 * segment.  d_halo and d_halo_len are read by the kernels, in stream order: a
 * copy or collective the caller enqueued on `stream` before the call is seen,
 * and the call makes no host synchronisation on their account.  Chained
 * scheme: a NULL d_halo or d_halo_len with n > 0 is DGPU_EINVAL.  The
 * unchained and G1-signature schemes never touch the two pointers (they may
 * be NULL).  n = 0 is a no-op that accepts NULL pointers.  RLC mode below
 * DGPU_RLC_MIN rounds runs per round, as elsewhere.  Measured on one GPU
 * only, like every multi-GPU path here: RCCL with two or more real ranks is
 * unmeasured. */
int dgpu_verify_segment_shard_device(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len,
                                     uint64_t first_round, size_t n, const uint8_t *d_sigs, size_t sig_stride,
                                     const uint32_t *d_sig_len, const uint8_t *d_halo, const uint32_t *d_halo_len,
                                     int mode, uint64_t rlc_seed, uint8_t *d_verdict_bits, uint8_t *d_reason,
                                     uint8_t *d_randomness32, void *stream);

/* Per-rank RLC protocol for callers that run one process (or one context)
 * per GPU and exchange data themselves -- the multi-process form of
 * dgpu_verify_multi's RLC mode (chain/beacon/sync_manager.go:188-222 sharded
 * by round range):
 *   1. dgpu_rlc_root_device: hash, decode (+ subgroup) and the bucket-MSM
 *      root of this rank's shard (device records as
 *      dgpu_verify_beacons_device) into d_root (dgpu_rlc_root_bytes(scheme)
 *      bytes of device memory: two Jacobian points of the signature group);
 *      the shard's points stay in the context.  rlc_seed must differ per rank
 *      (and be unpredictable to the beacons' producer).
 *   2. the caller all-gathers the ranks' roots (RCCL / any transport) into
 *      n_roots contiguous roots in device memory;
 *   3. dgpu_rlc_finish_device: sums the roots and checks the node (one
 *      pairing check); when it fails, descends this shard's tree; writes the
 *      shard's verdict bits (and reasons) exactly as dgpu_verify_beacons_device.
 * Every rank sees the same node verdict (the same roots, summed in order).
 * Any other verify / recovery call on the context between 1 and 3 cancels
 * the pending root (step 3 then fails with DGPU_EINVAL).  Synchronizes the
 * stream in step 3 (node verdict) like RLC mode does. */
int dgpu_rlc_root_bytes(int scheme);
int dgpu_rlc_root_device(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n,
                         const uint64_t *d_rounds, const uint8_t *d_sigs, size_t sig_stride, const uint32_t *d_sig_len,
                         const uint8_t *d_prev, size_t prev_stride, const uint32_t *d_prev_len, uint64_t rlc_seed,
                         uint8_t *d_root, void *stream);
int dgpu_rlc_finish_device(dgpu_ctx *ctx, size_t n_roots, const uint8_t *d_roots, uint8_t *d_verdict_bits,
                           uint8_t *d_reason, void *stream);
/* Step 1 of the per-rank RLC protocol over a linked shard; steps 2-3 are
 * unchanged (the all-gather, dgpu_rlc_finish_device).  d_halo != NULL: the
 * halo form of dgpu_verify_segment_shard_device (seed_prev is ignored);
 * d_halo == NULL: the host seed by value, as dgpu_verify_segment_device (the
 * rank that holds the segment's first round).  The pending root keeps the
 * source, halo pointers included: they stay valid until
 * dgpu_rlc_finish_device, as d_sigs already must.  Everything else is
 * dgpu_rlc_root_device's: any other call cancels the pending root, n = 0
 * yields the identity root, rlc_seed is per rank, and the finish step's
 * verdicts equal dgpu_verify_segment_shard_device's on the shard.  The
 * protocol returns no randomness (a walk needs it for the one round it
 * returns).  RCCL with two or more real ranks is unmeasured. */
int dgpu_rlc_root_segment_device(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, uint64_t first_round,
                                 size_t n, const uint8_t *d_sigs, size_t sig_stride, const uint32_t *d_sig_len,
                                 const uint8_t *seed_prev, size_t seed_prev_len, const uint8_t *d_halo,
                                 const uint32_t *d_halo_len, uint64_t rlc_seed, uint8_t *d_root, void *stream);

/* Batch key.Scheme.VerifyRecovered(pk, msg, sig) (= bls.Verify (R); call
 * sites chain/verify.go:44, chain/beacon/chain.go:165; AuthScheme
 * key/curve.go:39) over raw messages of any length: message i is msg_len[i]
 * bytes at msgs + i*msg_stride (msg_len[i] <= msg_stride, else DGPU_EINVAL).
 * Signatures, key, mode and outputs as dgpu_verify_beacons. */
int dgpu_verify_recovered(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t pk_len, size_t n,
                          const uint8_t *msgs, size_t msg_stride, const uint32_t *msg_len, const uint8_t *sigs,
                          size_t sig_stride, const uint32_t *sig_len, int mode, uint64_t rlc_seed,
                          uint8_t *verdict_bits, uint8_t *reason);

/* Batch form of bls.Verify(keys[key_idx[i]], msg_i, sig_i): every record under
 * its own key.  Call sites: Identity.ValidSignature / Group.UnsignedIdentities
 * (key/keys.go:52-63, key/group.go:474-482; core/group_setup.go:187,
 * core/drand_beacon.go:85) -- AuthScheme.Verify(node.Key, blake2b-256(node.Key),
 * node.Signature), one key per node, under DGPU_SCHEME_CHAINED's groups and
 * DST (AuthScheme, key/curve.go:39) --, and a relay or gossip validator that
 * follows several chains and verifies their records in one call.
 * Messages and signatures are exactly dgpu_verify_recovered's (raw messages of
 * any length; msg_len[i] > msg_stride is DGPU_EINVAL); `scheme` selects the
 * groups and the hash DST as there.
 * keys: a host pointer in both forms, n_keys x key_len bytes of compressed
 * keys; key_len is 48 for the G2-signature schemes and 96 for the G1-signature
 * schemes (any other value: DGPU_EINVAL); 1 <= n_keys <= 65536 (else
 * DGPU_EINVAL).  The table is copied before the call returns (like pk and
 * seed_prev) and decoded on the device with the rules of dgpu_decode_pubkey.
 * A rejected key is not an argument error: every record naming it gets
 * verdict 0 and DGPU_REASON_KEY, which takes precedence over the record's own
 * signature reason (the reference decodes the key before it looks at the
 * signature).  The decode result is never read back by the host: the device
 * form stays asynchronous.
 * key_idx[i] >= n_keys: the host form returns DGPU_EINVAL before any device
 * work; the device form gives the record DGPU_REASON_KEY and reads nothing
 * outside the table.
 * Contract: verdict bits and reasons equal dgpu_verify_recovered called once
 * per key on that key's records under the same scheme and mode -- that call's
 * reasons for a valid key, DGPU_REASON_KEY where that call returns DGPU_EINVAL.
 * mode: DGPU_MODE_PER_ROUND (one pairing check per record, each against its
 * own key, in one pairing batch on one stream) or DGPU_MODE_RLC (any other
 * value: DGPU_EINVAL).  RLC mode applies at n >= DGPU_RLC_MIN records; below
 * that the call runs per record, as elsewhere.  A batch under K keys splits
 * into K independent random linear combinations: per record the leaves
 * [a_i] H(m_i) + [b_i] endo(H(m_i)) and the same of sig_i, (a_i, b_i) the
 * halves of the 64-bit coefficient derived from rlc_seed and i; per key the
 * sums of its undecided records' leaves; one 2-pairing check per non-empty
 * key.  The records of every failing key are then checked one by one, exactly
 * (bisection inside a key's group is not built: one bad record costs its
 * key's whole group a per-record pass), so verdicts and reasons equal
 * per-record mode's except with probability <= 2^-64 per failing check.
 * Signatures are subgroup-checked before any combination and table keys at
 * decode.  RLC mode synchronises the stream once (the count of records left
 * to the exact check), as the single-key RLC mode does for its node verdict.
 * Cost: a record's pairing check is replaced by two 64-bit scalar
 * multiplications in the signature group (measured at 1Mi records: about 70 ms
 * against 340 ms of pairing checks for G2 signatures, 22 ms for G1
 * signatures), and every non-empty key adds one pairing check, every failing
 * key a per-record pass over its records (profiles/r16/keyed_vs_calls.txt).
 * Clean batches of 1Mi records were faster in RLC mode at every table size
 * measured, K = 1 to 65,536 (1.7-2.1 times for G2 signatures, 3.3-4.5 times
 * for G1 signatures).  Stay per record when K approaches n (node identities:
 * one record per key, nothing to combine) and when most keys are expected to
 * hold a bad record: the combination is then paid on top of the per-record
 * pass (with 0.1% corrupted, RLC mode was 1.3 times slower than per record at
 * K <= 8 and no faster at K = 1,024 for G2 signatures).  A dirty batch under
 * one key is dgpu_verify_recovered's case, whose RLC mode bisects.
 * n = 0 is a no-op that accepts NULL pointers; any keyed call cancels a
 * pending RLC root, like every other call.  The whole call runs on one stream.
 * The host form stages its records through the pinned ring, the key indices
 * as one more 4-byte array behind the records; dgpu_staging_stats bytes are
 * n x (msg_stride + sig_stride + 12). */
int dgpu_verify_keyed(dgpu_ctx *ctx, int scheme, size_t n_keys, const uint8_t *keys, size_t key_len, size_t n,
                      const uint32_t *key_idx, const uint8_t *msgs, size_t msg_stride, const uint32_t *msg_len,
                      const uint8_t *sigs, size_t sig_stride, const uint32_t *sig_len, int mode, uint64_t rlc_seed,
                      uint8_t *verdict_bits, uint8_t *reason);

/* dgpu_verify_keyed over device-resident records (d_* are device pointers;
 * keys stays a host pointer), asynchronous on `stream` as
 * dgpu_verify_beacons_device.  A record with d_msg_len[i] > msg_stride is not
 * read past its stride and fails with DGPU_REASON_DECODE. */
int dgpu_verify_keyed_device(dgpu_ctx *ctx, int scheme, size_t n_keys, const uint8_t *keys, size_t key_len, size_t n,
                             const uint32_t *d_key_idx, const uint8_t *d_msgs, size_t msg_stride,
                             const uint32_t *d_msg_len, const uint8_t *d_sigs, size_t sig_stride,
                             const uint32_t *d_sig_len, int mode, uint64_t rlc_seed, uint8_t *d_verdict_bits,
                             uint8_t *d_reason, void *stream);

/* Batch form of Verifier.VerifyBeacon (chain/verify.go:38-45) over n beacons
 * given as fixed-stride records (host pointers):
 *   rounds[i]                   Beacon.Round
 *   sigs + i*sig_stride         Beacon.Signature, sig_len[i] bytes (any length
 *                               != 96 -- != 48 for the G1-signature schemes --
 *                               is a decode failure, like the reference)
 *   prev + i*prev_stride        Beacon.PreviousSig, prev_len[i] <= prev_stride
 *                               bytes; ignored (may be NULL) for unchained schemes
 * mode: DGPU_MODE_PER_ROUND (one pairing check per round) or DGPU_MODE_RLC
 *       (random linear combination over the batch with coefficients derived
 *       from rlc_seed, exact per-round verdicts by bisection; the verdicts are
 *       identical to per-round mode except with probability <= 2^-64 per
 *       failing check; pass a fresh unpredictable seed for adversarial input;
 *       every scheme: G2 signatures and the G1-signature schemes, whose
 *       node checks run on the key's fixed-Q line table).  The scheme must sign on the same group as
 *       the installed key's scheme (else DGPU_ENOKEY).
 * verdict_bits: ceil(n/8) bytes out.  reason: optional n bytes out. */
int dgpu_verify_batch(dgpu_ctx *ctx, int scheme, size_t n, const uint64_t *rounds, const uint8_t *sigs,
                      size_t sig_stride, const uint32_t *sig_len, const uint8_t *prev, size_t prev_stride,
                      const uint32_t *prev_len, int mode, uint64_t rlc_seed, uint8_t *verdict_bits,
                      uint8_t *reason);

/* Same contract with every array already resident in device memory of the
 * context's GPU (d_* are device pointers) and work enqueued on `stream`
 * (a hipStream_t, NULL = the legacy default stream).  Asynchronous: results
 * are valid after the stream synchronizes (or dgpu_synchronize returns). */
int dgpu_verify_batch_device(dgpu_ctx *ctx, int scheme, size_t n, const uint64_t *d_rounds, const uint8_t *d_sigs,
                             size_t sig_stride, const uint32_t *d_sig_len, const uint8_t *d_prev,
                             size_t prev_stride, const uint32_t *d_prev_len, int mode, uint64_t rlc_seed,
                             uint8_t *d_verdict_bits, uint8_t *d_reason, void *stream);

/* Instrumentation: when enabled, every verify call records one HIP event
 * per kernel stage on the stream it runs on; dgpu_stage_times writes the
 * stage durations (ms) and names of the last call, summed per name over
 * chunks (per-round mode: hash_to_g2, h_affine, decode_g2, eng_lines,
 * eng_miller, eng_inv, eng_fe, eng_fe_chain, eng_fe_kbinv, pack_verdicts,
 * randomness (dgpu_verify_segment with a randomness buffer); G1
 * signatures: hash_to_g1, h_affine, decode_g1, eng_miller (eng_lines_fixed
 * first under DGPU_G1_LINES=buffer), ...; RLC mode: rlc_hash_to_g2_raw /
 * rlc_hash_to_g1_raw, decode_g2 / decode_g1, rlc_affine, rlc_root_msm,
 * rlc_prep, the engine stages of the node checks, rlc_leaves_tree,
 * rlc_bisection; recovery: recover_hash, recover_decode, recover_select,
 * recover_lagrange, engine stages, recover_msm, recover_rlc_g1 (a
 * G1-signature group: recover_rlc_g2), recover_verdict; keyed calls: keyed_keys (the table's
 * upload and decode), the hash and decode stages, keyed_gather, the engine
 * stages, pack_verdicts, and in RLC mode keyed_leaves, keyed_group, keyed_sums,
 * keyed_prep ahead of the node checks' engine stages and keyed_fallback -- only
 * when a key failed -- around the exact check's; dgpu_verify_partials: recover_hash, recover_decode,
 * the engine stages, pack_verdicts), at most max_stages of them, and returns the
 * number of distinct stages the call recorded (like snprintf: a value above
 * max_stages means the output was truncated).  DGPU_MAX_STAGES bounds every
 * pipeline's count.  A call that recorded more stage events than the
 * library's event pool holds makes dgpu_stage_times fail (DGPU_EINVAL)
 * instead of reporting partial sums. */
#define DGPU_MAX_STAGES 32
/* Block until every call made so far on the context has finished on the
 * device (its results are then valid on the host and on any stream). */
int dgpu_synchronize(dgpu_ctx *ctx);
int dgpu_set_profiling(dgpu_ctx *ctx, int enable);
/* Host-record staging of the last call on the context that took host records
 * (dgpu_verify_beacons, dgpu_verify_batch, dgpu_verify_recovered, dgpu_verify_keyed, a shard of
 * dgpu_verify_multi or dgpu_verify_segment_multi) or stored rows
 * (dgpu_verify_rows, dgpu_check_rows, a shard of dgpu_check_rows_multi: their
 * bytes are stated there): the records go through a library-owned pinned ring
 * (two 16 MiB slots per context, filled by host threads, DMA'd on the
 * context's copy stream) slice by slice, each slice's kernels starting when
 * its records have arrived.  device_ms = the staging's span on the copy
 * stream, first piece to last DMA (device timeline); host_ms = the staging
 * thread's wall time, first memcpy into the ring to the last DMA enqueued;
 * bytes = record bytes staged. */
int dgpu_staging_stats(dgpu_ctx *ctx, double *device_ms, double *host_ms, uint64_t *bytes);
int dgpu_stage_times(dgpu_ctx *ctx, float *ms_out, int max_stages, const char **names_out);

/* Batch DigestMessage (chain/verify.go:24-32): out32 = n x 32 bytes. */
int dgpu_digest_batch(dgpu_ctx *ctx, int scheme, size_t n, const uint64_t *rounds, const uint8_t *prev,
                      size_t prev_stride, const uint32_t *prev_len, uint8_t *out32);

/* Hash to the scheme's signature group of n raw messages of any length
 * (msg_len[i] <= msg_stride): 96-byte compressed G2 points under drand's G2
 * DST (kyber G2 Hash (R), pinned by key/curve_test.go:10-30), or 48-byte
 * compressed G1 points for the G1-signature schemes. */
int dgpu_hash_to_curve(dgpu_ctx *ctx, int scheme, size_t n, const uint8_t *msgs, size_t msg_stride,
                       const uint32_t *msg_len, uint8_t *out);

/* Sign n raw messages with a 32-byte big-endian secret (< r): sig = sk *
 * H(msg), compressed (96 bytes on G2, 48 on G1 for the G1-signature
 * schemes).  Test/tool surface of key.Scheme.Sign / AuthScheme.Sign
 * (key/curve.go:36-39), as key/curve_test.go:10-30 uses it. */
int dgpu_sign(dgpu_ctx *ctx, int scheme, const uint8_t *sk_be32, size_t n, const uint8_t *msgs, size_t msg_stride,
              const uint32_t *msg_len, uint8_t *out_sigs);

/* Decode n 48-byte compressed G1 points (public keys, commitments:
 * chain/convert.go:20-23, key/group.go TOML keys) with kilic's
 * FromCompressed rules (R) + subgroup check: rc_out[i] = 0 decoded, 4 the
 * point at infinity, other values an error (flags, x >= p, not on the curve,
 * not in the subgroup); xy96 (optional) = canonical big-endian x || y. */
int dgpu_decode_g1_points(dgpu_ctx *ctx, size_t n, const uint8_t *in48, int *rc_out, uint8_t *xy96);

/* The scheme's signature decoder alone (Beacon.Signature -> SigGroup point:
 * the UnmarshalBinary inside bls.Verify (R), chain/verify.go:44): n records
 * as in dgpu_verify_beacons (sig_len[i] bytes at sigs + i*sig_stride; any
 * length other than 48 -- G1-signature schemes -- or 96 is a decode error),
 * decoded with the subgroup check by the same kernels the verify paths run
 * (k_decode_g1_sigs; k_decode_g2_sigs_sub).  reason: n bytes of
 * DGPU_REASON_DECODE / _SUBGROUP / _INFINITY or 0; xy (optional): canonical
 * big-endian affine coordinates, 96 bytes per record on G1 (x || y) and 192
 * on G2 (x.c0 || x.c1 || y.c0 || y.c1), zero unless the record decoded. */
int dgpu_decode_signatures(dgpu_ctx *ctx, int scheme, size_t n, const uint8_t *sigs, size_t sig_stride,
                           const uint32_t *sig_len, uint8_t *reason, uint8_t *xy);

/* The scheme's public-key decoder (chain.Info.PublicKey, chain/convert.go:20-23;
 * the decode dgpu_set_pubkey / dgpu_verify_beacons run on a key-cache miss):
 * 48-byte compressed G1 for the G2-signature schemes, 96-byte compressed G2
 * for the G1-signature schemes, subgroup-checked.  DGPU_EINVAL if rejected;
 * xy (optional): the affine point as dgpu_decode_signatures writes it (96
 * bytes for a G1 key, 192 for a G2 key).  The key cache is not touched. */
int dgpu_decode_pubkey(dgpu_ctx *ctx, int scheme, const uint8_t *pk, size_t len, uint8_t *xy);

/* Hash-to-G2 of n 32-byte messages with drand's DST (kyber G2 Hash (R)),
 * compressed to 96 bytes each: the parity surface for hash-to-curve. */
int dgpu_hash_to_g2(dgpu_ctx *ctx, size_t n, const uint8_t *msg32, uint8_t *out96);

/* Hash-to-G1 of n 32-byte messages (RFC 9380 suite BLS12381G1_XMD:SHA-256_
 * SSWU_RO_) with the DST of a G1-signature scheme, compressed to 48 bytes. */
int dgpu_hash_to_g1(dgpu_ctx *ctx, int scheme, size_t n, const uint8_t *msg32, uint8_t *out48);

/* pk = sk * g1 (48-byte compressed G1; 96-byte sk * g2 for the G1-signature
 * schemes) for a 32-byte big-endian secret: synthetic-chain tool
 * (KeyGroup.Point().Mul(secret, nil), client/test/result/mock/result.go:88). */
int dgpu_derive_pubkey(dgpu_ctx *ctx, int scheme, const uint8_t *sk_be32, uint8_t *pk_out, size_t pk_len);

/* Threshold group public polynomial share.PubPoly (kyber (R); key/keys.go
 * DistPublic.Coefficients, chain/beacon/node.go:117-125 uses it through
 * key.Scheme.VerifyPartial): t compressed G1 commitments C_0..C_{t-1}
 * (48 bytes each), group size n (share indices 0..n-1 get a precomputed
 * PubPoly.Eval table; larger indices are evaluated on the fly).
 * 1 <= t <= 32, t <= n <= 65536.  Rejects undecodable commitments.
 * Installs a G2-signature group (the two pedersen-bls schemes).  drand's
 * key.MinimumT is n/2 + 1, so t <= 32 serves groups of up to 63 nodes: larger
 * groups are installed with dgpu_set_group_wide. */
int dgpu_set_group(dgpu_ctx *ctx, int t, int n, const uint8_t *commits48);

/* dgpu_set_group for any scheme.  DGPU_SCHEME_CHAINED / _UNCHAINED:
 * commit_len must be 48 and the call is exactly dgpu_set_group.
 * DGPU_SCHEME_UNCHAINED_G1 / _G1_RFC9380 (signatures on G1, keys on G2, the
 * same key.Scheme.Recover / VerifyPartial call sites): commit_len must be 96,
 * the commitments are compressed G2 points C_j = a_j g2, decoded with kilic's
 * rules and the subgroup check; the PubPoly.Eval table is built in G2 and C_0
 * is installed as VerifyRecovered's key (its fixed Miller-loop lines, as
 * dgpu_set_pubkey computes them, outside the 8-entry key cache).  The group
 * remembers its scheme: it selects the hash DST and the partial format of the
 * recover entry points.  Same limits on t and n.  DGPU_EINVAL for a wrong
 * commit_len, an unknown scheme, or an undecodable or out-of-subgroup
 * commitment; a rejected G1-signature call leaves the installed group as it
 * was. */
int dgpu_set_group_scheme(dgpu_ctx *ctx, int scheme, int t, int n, const uint8_t *commits, size_t commit_len);

/* The largest threshold of dgpu_set_group_wide (groups of up to 2047 nodes
 * under key.MinimumT). */
#define DGPU_MAX_THRESHOLD 1024

/* dgpu_set_group_scheme without its limit on t: 1 <= t <= DGPU_MAX_THRESHOLD,
 * t <= n <= 65536.  For t <= 32 the call is exactly dgpu_set_group_scheme.
 * Above, the same group state is built under the same rules (commitment
 * decoding, subgroup checks, which rejected calls keep the installed group),
 * and the recover and partial entry points (dgpu_recover_batch[_device],
 * dgpu_recover_multi, dgpu_verify_partials[_device]) take their wide path:
 * the same results by kernels that share a round's t terms among lanes
 * (one Fr inversion per round for the Lagrange coefficients, L lanes per
 * multi-scalar slice) and build the window tables of a batch in chunks of
 * rounds of at most 1 GiB (RECW_TABLE_BUDGET; 3,136 t bytes per round for G2
 * signatures, 1,792 t for G1), enqueued in order on the call's stream.
 * Installing is O(n t) point operations per table. */
int dgpu_set_group_wide(dgpu_ctx *ctx, int scheme, int t, int n, const uint8_t *commits, size_t commit_len);

/* Batch form of key.Scheme.Recover (kyber tbls.Recover + share.RecoverCommit
 * (R)) as the aggregator calls it (chain/beacon/chain.go:158-168), n_rounds
 * rounds at once.  Round r signs msgs32 + 32 r (its DigestMessage) and offers
 * m partial slots: partial j is partials + (r m + j) partial_stride, length
 * partial_len[r m + j] (0 = empty slot); a partial is BE16(share index) ||
 * 96-byte G2 signature (tbls.Sign).  Per round, exactly like the reference:
 * partials are walked in order, those with a readable index that pass
 * VerifyPartial (decode + subgroup + pairing against PubPoly.Eval(index))
 * are kept until t are kept; duplicates of an index count once; fewer than t
 * distinct -> the reference's error (bit 0 in ok_bits, zero signature);
 * otherwise out_sigs + 96 r = the Lagrange-interpolated signature, kept
 * only if it passes VerifyRecovered under C_0 (chain.go:165), as the
 * aggregator does before appending the beacon.
 * partial_valid (optional, n_rounds*m bytes): 1 iff the partial verified.
 * The call follows the installed group's scheme.  Under a G1-signature group
 * (dgpu_set_group_scheme) a partial is BE16(share index) || 48-byte G1
 * signature, 50 bytes -- any other length, 98 included, is a decode error --,
 * messages are hashed to G1 under the scheme's DST, partial_stride >= 50, and
 * the recovered signature of round r is 48 bytes at out_sigs + 48 r (zero on
 * failure); everything else as above.  out_sigs: n_rounds * 96 bytes for a
 * G2-signature group, n_rounds * 48 for a G1-signature group. */
int dgpu_recover_batch(dgpu_ctx *ctx, size_t n_rounds, const uint8_t *msgs32, size_t m, const uint8_t *partials,
                       size_t partial_stride, const uint32_t *partial_len, uint8_t *out_sigs, uint8_t *ok_bits,
                       uint8_t *partial_valid);

/* dgpu_recover_batch over device buffers already resident in HBM, enqueued on
 * `stream` (hipStream_t; NULL = the legacy default stream) without host
 * synchronisation.  d_ok: n_rounds bytes (1 = recovered); d_status
 * (optional): n_rounds*m bytes, DGPU_REASON_* of every partial (0 = verified).
 * A partial_len above partial_stride reads as an invalid partial.
 * d_out_sigs: 96 bytes per round, 48 under a G1-signature group. */
int dgpu_recover_batch_device(dgpu_ctx *ctx, size_t n_rounds, const uint8_t *d_msgs32, size_t m,
                              const uint8_t *d_partials, size_t partial_stride, const uint32_t *d_partial_len,
                              uint8_t *d_out_sigs, uint8_t *d_ok, uint8_t *d_status, void *stream);

/* key.Scheme.VerifyPartial of every slot of dgpu_recover_batch's input shape
 * under the installed group (DGPU_ENOKEY without one), as the node runs it on
 * a partial's arrival (chain/beacon/node.go:117-125) -- which partials verify,
 * without a recovery.  The item key is PubPoly.Eval(index): from the group's
 * table for index < n, evaluated on the fly above it.  Partials are in the
 * installed group's format (98 bytes, or 50 under a G1-signature group).
 * valid_bits: one bit per slot, ceil(n_rounds m / 8) bytes, slot r m + j at bit
 * (r m + j) % 8 of byte (r m + j) / 8; reason (optional, n_rounds m bytes): the
 * DGPU_REASON_* of that partial alone.  There is no "stop after t" and no
 * duplicate rule; an empty or mis-sized slot (a length above the stride
 * included, which is never read) is DGPU_REASON_DECODE.  It is the first step
 * of the exact recovery path (hash, partial decode, one pairing per partial)
 * followed by the verdict pack.  mode: DGPU_MODE_PER_ROUND or DGPU_MODE_RLC (any
 * other value: DGPU_EINVAL).  RLC mode, at DGPU_RLC_MIN slots and above, is
 * dgpu_verify_keyed's per-key combination with the share index as the key
 * index: one 2-pairing check per share that has an undecided partial, the
 * round's hash point shared by the round's slots, then the exact check of
 * every failing share's partials.  A partial whose index lies above the
 * group's table (its key evaluated on the fly) is not combined: it goes to the
 * exact check.  Verdicts and reasons equal per-record mode's except with
 * probability <= 2^-64 per failing check; pass a fresh unpredictable
 * rlc_seed (partials come from peers).  One stream synchronisation, as there.  n_rounds = 0 is a no-op that accepts
 * NULL pointers. */
int dgpu_verify_partials(dgpu_ctx *ctx, size_t n_rounds, const uint8_t *msgs32, size_t m, const uint8_t *partials,
                         size_t partial_stride, const uint32_t *partial_len, int mode, uint64_t rlc_seed,
                         uint8_t *valid_bits, uint8_t *reason);

/* dgpu_verify_partials over device buffers, asynchronous on `stream` (as
 * dgpu_recover_batch_device). */
int dgpu_verify_partials_device(dgpu_ctx *ctx, size_t n_rounds, const uint8_t *d_msgs32, size_t m,
                                const uint8_t *d_partials, size_t partial_stride, const uint32_t *d_partial_len,
                                int mode, uint64_t rlc_seed, uint8_t *d_valid_bits, uint8_t *d_reason, void *stream);

/* Synthetic threshold partials (test/bench data tool; tbls.Sign (R),
 * chain/beacon/node_test.go:56-106 builds the same shape): for item i of
 * round i / m, out98 + 98 i = BE16(label[i]) || compress(share[sign_idx[i]] *
 * H(msgs32 + 32 (i / m))), shares given as 32-byte big-endian scalars
 * (n_shares of them).  A label different from the signing share's index
 * yields an invalid partial. */
int dgpu_make_partials(dgpu_ctx *ctx, size_t n_rounds, const uint8_t *msgs32, size_t m, const uint32_t *sign_idx,
                       const uint32_t *label, const uint8_t *shares_be32, size_t n_shares, uint8_t *out98);

/* dgpu_make_partials for any scheme: the G1-signature schemes write 2 + 48
 * bytes per item, BE16(label[i]) || compress(share * H_G1(msg)) under the
 * scheme's DST, at out + 50 i; the other schemes 98 bytes as above. */
int dgpu_make_partials_scheme(dgpu_ctx *ctx, int scheme, size_t n_rounds, const uint8_t *msgs32, size_t m,
                              const uint32_t *sign_idx, const uint32_t *label, const uint8_t *shares_be32,
                              size_t n_shares, uint8_t *out);

/* Synthetic chain generator (test/bench data tool; mirrors the reference's
 * fixture generator client/test/result/mock/result.go:86-130).  Builds
 * n_seg independent segments of seg_len rounds each, signed with the 32-byte
 * big-endian secret scalar sk_be32 (< r):
 *   segment s covers rounds first_round[s] .. first_round[s] + seg_len - 1;
 *   its first round's PreviousSig is seed_prev + s*96 (seed_prev_len[s]
 *   bytes), every later round's PreviousSig is the previous signature.
 * Output (host pointers): sigs_out[(s*seg_len + j)*96 ...] for round
 * first_round[s] + j.  Unchained schemes ignore the previous signature. */
int dgpu_make_chain(dgpu_ctx *ctx, int scheme, const uint8_t *sk_be32, size_t n_seg, size_t seg_len,
                    const uint64_t *first_round, const uint8_t *seed_prev, const uint32_t *seed_prev_len,
                    uint8_t *sigs_out);

/* ---------------------------------------------------------------- multi-GPU
 * One handle over ndev GPUs of a node: a context per device
 * and an RCCL communicator over them (ncclCommInitAll; RCCL is loaded when
 * the handle opens, DGPU_EUNSUPPORTED without it).  dgpu_verify_multi is
 * dgpu_verify_beacons over host records sharded contiguously across the
 * devices (dgpu_shard_range), as the bulk check-chain loop would call it
 * (chain/beacon/sync_manager.go:188-222): the data path has no collective;
 * RCCL all-gathers the per-device verdict bitmaps (and reasons), and in RLC
 * mode first the per-device RLC roots, checked once on the first device --
 * one final exponentiation for the whole batch when every round is valid.
 * Verdicts equal dgpu_verify_beacons' on the same records. */
typedef struct dgpu_multi dgpu_multi;
int dgpu_multi_open(int ndev, const int *devs, dgpu_multi **out);
void dgpu_multi_close(dgpu_multi *m);
/* the k-th device's context (owned by the handle) */
int dgpu_multi_context(dgpu_multi *m, int k, dgpu_ctx **out);
int dgpu_verify_multi(dgpu_multi *m, int scheme, const uint8_t *pk, size_t pk_len, size_t n, const uint64_t *rounds,
                      const uint8_t *sigs, size_t sig_stride, const uint32_t *sig_len, const uint8_t *prev,
                      size_t prev_stride, const uint32_t *prev_len, int mode, uint64_t rlc_seed,
                      uint8_t *verdict_bits, uint8_t *reason);

/* dgpu_verify_segment over the devices of a multi handle: arguments and
 * results exactly as dgpu_verify_segment on one context (verdict bits,
 * reasons and randomness, bit for bit, in both modes).  The shards follow
 * dgpu_shard_range.  Shard 0 takes the caller's seed, by value; shard k > 0
 * takes record lo_k - 1 of the caller's arrays as its halo
 * (dgpu_verify_segment_shard_device): the library stages that record and its
 * length into a small per-context buffer ahead of the shard's own records.
 * Each shard's signatures go through its context's pinned ring once --
 * n_k x (sig_stride + 4) bytes, which is what dgpu_staging_stats reports for
 * the context; the halo's sig_stride + 4 bytes are staged beside them and are
 * not counted in that figure.  Modes, per-device RLC seeds, the root
 * all-gather and single check, the per-shard descent and the bitmap / reason
 * gathers are dgpu_verify_multi's (the same code).  The randomness is
 * computed per shard once the shard's statuses are final and goes from each
 * device straight to randomness32 + 32 lo_k.  RCCL with two or more real
 * ranks is unmeasured. */
int dgpu_verify_segment_multi(dgpu_multi *m, int scheme, const uint8_t *pk, size_t pk_len, uint64_t first_round,
                              size_t n, const uint8_t *sigs, size_t sig_stride, const uint32_t *sig_len,
                              const uint8_t *seed_prev, size_t seed_prev_len, int mode, uint64_t rlc_seed,
                              uint8_t *verdict_bits, uint8_t *reason, uint8_t *randomness32);

/* dgpu_check_rows over the devices of a multi handle: the same arguments and
 * the same results, element for element, in both modes.  The rows shard by
 * dgpu_shard_range(n, D, k); each shard's rows and keys go through its
 * context's ring and row decoder (dgpu_staging_stats of that context: the
 * shard's bytes by dgpu_check_rows' formula).  The RLC phases are
 * dgpu_verify_multi's unchanged: per-device seeds, the root all-gather, one
 * check, the per-shard descent.  Each device builds the list of the
 * positions it owns: shard 0 from position 0, a later non-empty shard k from
 * keys[lo_k] - first, the last non-empty shard up to count (a run of missing
 * rounds in front of a shard's first key belongs to the shard before it; with
 * n = 0 shard 0 owns everything).  The host concatenates the per-device lists
 * in shard order, left-row indices made global; no collective carries them,
 * and no verdict bitmap is gathered (the reasons only when `reason` is
 * given).  RCCL with two or more real ranks is unmeasured. */
int dgpu_check_rows_multi(dgpu_multi *m, int scheme, const uint8_t *pk, size_t pk_len, size_t n, const uint8_t *base,
                          const uint64_t *row_off, const uint32_t *row_len, const uint64_t *keys, size_t sig_stride,
                          size_t prev_stride, int mode, uint64_t rlc_seed, uint64_t first, size_t count,
                          uint64_t *faulty_pos, uint64_t *faulty_val, size_t faulty_cap, uint64_t *n_faulty,
                          uint64_t *left_rows, size_t left_cap, uint64_t *n_left, uint8_t *reason);

/* dgpu_set_group on every device of the handle (the aggregator's group,
 * chain/beacon/chain.go:158-168 -> key.Scheme.Recover). */
int dgpu_multi_set_group(dgpu_multi *m, int t, int n, const uint8_t *commits48);
/* dgpu_set_group_scheme on every device of the handle. */
int dgpu_multi_set_group_scheme(dgpu_multi *m, int scheme, int t, int n, const uint8_t *commits, size_t commit_len);
/* dgpu_set_group_wide on every device of the handle. */
int dgpu_multi_set_group_wide(dgpu_multi *m, int scheme, int t, int n, const uint8_t *commits, size_t commit_len);

/* dgpu_recover_batch over the node: rounds shard contiguously across the
 * devices (dgpu_shard_range over n_rounds), each device recovers its shard,
 * RCCL all-gathers the per-device recovery bitmaps; recovered signatures and
 * per-partial validity go to the host from the device that computed them.
 * Arguments and results exactly as dgpu_recover_batch (out_sigs: 96 bytes per
 * round, 48 under a G1-signature group). */
int dgpu_recover_multi(dgpu_multi *m, size_t n_rounds, const uint8_t *msgs32, size_t m_slots, const uint8_t *partials,
                       size_t partial_stride, const uint32_t *partial_len, uint8_t *out_sigs, uint8_t *ok_bits,
                       uint8_t *partial_valid);

/* Test mode (environment, read by dgpu_multi_open): DGPU_MULTI_ALLOW_SAME_DEVICE=1
 * lets devs list one GPU several times (one context each) and replaces the
 * RCCL all-gathers with in-library device copies, so one GPU runs every
 * multi-device branch (shard padding, per-device seeds, root sum). */

#ifdef __cplusplus
}
#endif
#endif /* DRAND_GPU_H */
