"""Host-side mirror of drand's chain verification surface, backed by the
MI355X kernels through the C-ABI (include/drand_gpu.h).

Mirrors (same names, argument meaning and error behaviour):
  chain.Beacon                      chain/beacon.go:13-20  (+ Randomness :51-54)
  chain.RoundToBytes                chain/store.go:42-46
  chain.NewVerifier / Verifier      chain/verify.go:13-49
      DigestMessage(round, prevSig) chain/verify.go:24-32
      VerifyBeacon(b, pubkey) error chain/verify.go:38-45
      IsPrevSigMeaningful()         chain/verify.go:47-49
and adds the batch form every bulk caller needs (sync_manager.go:188-222,
client/verify.go:149-169): Verifier.verify_beacons(beacons, pubkey).

There is no CPU fallback: every digest and every verification runs on the
GPU; constructing a Verifier without the HIP library or a gfx950 device
raises DrandGPUError.
"""
import hashlib
import struct
import threading
from dataclasses import dataclass

import numpy as np

from . import _lib, calls
from .calls import pack_msgs as _pack_msgs, rlc_seed_for  # noqa: F401  (their callers import them from here)
from .scheme import Scheme, scheme_code


class VerifyError(Exception):
    """Non-nil error of VerifyBeacon; `reason` is the DGPU_REASON_* code."""

    MESSAGES = {
        _lib.REASON_DECODE: "bls: invalid signature encoding",
        _lib.REASON_SUBGROUP: "bls: signature point is not on correct subgroup",
        _lib.REASON_PAIRING: "bls: invalid signature",
        _lib.REASON_INFINITY: "bls: invalid signature",
    }

    def __init__(self, round_, reason):
        super().__init__(f"round {round_}: {self.MESSAGES.get(reason, 'invalid beacon')}")
        self.round = round_
        self.reason = reason


@dataclass
class Beacon:
    """chain/beacon.go:13-20"""
    previous_sig: bytes
    round: int
    signature: bytes

    def randomness(self):
        """chain/beacon.go:43-45 (host bookkeeping, SHA-256 of the signature)."""
        return randomness_from_signature(self.signature)

    def get_round(self):
        return self.round


def round_to_bytes(r):
    """chain/store.go:42-46: 8-byte big-endian."""
    return struct.pack(">Q", r)


def randomness_from_signature(sig):
    """chain/beacon.go:51-54 (not part of the verify hot path)."""
    return hashlib.sha256(sig).digest()


_contexts = {}
_ctx_lock = threading.Lock()


def get_context(device=0):
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = _lib.Context(device)
            _contexts[device] = ctx
        return ctx


def pack_beacons(beacons, sig_stride=96, prev_stride=None):
    """Fixed-stride records for dgpu_verify_batch (numpy arrays)."""
    n = len(beacons)
    if prev_stride is None:
        prev_stride = max([96] + [len(b.previous_sig or b"") for b in beacons])
    rounds = np.fromiter((b.round for b in beacons), dtype=np.uint64, count=n)
    sig_len = np.fromiter((len(b.signature or b"") for b in beacons), dtype=np.uint32, count=n)
    prev_len = np.fromiter((len(b.previous_sig or b"") for b in beacons), dtype=np.uint32, count=n)
    stride = max(sig_stride, 96)
    sigs = np.zeros((n, stride), dtype=np.uint8)
    prev = np.zeros((n, prev_stride), dtype=np.uint8)
    for i, b in enumerate(beacons):
        s = b.signature or b""
        if 0 < len(s) <= stride:
            sigs[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
        elif len(s) > stride:
            sig_len[i] = 0xFFFFFFFF  # any length != 96 fails decode, like kilic (R)
        p = b.previous_sig or b""
        if p:
            prev[i, : len(p)] = np.frombuffer(p, dtype=np.uint8)
    return rounds, sigs, sig_len, prev, prev_len


class RecordCalls:
    """The batch surface that Verifier and multi.MultiVerifier share: the same
    packing and checks over `self.ctx`, under the single or the multi form of
    each entry point."""

    _records = staticmethod(calls.verify_beacons)
    _segment = staticmethod(calls.verify_segment)
    _rows = staticmethod(calls.check_rows)

    def verify_reasons(self, beacons, pubkey, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        n = len(beacons)
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        rounds, sigs, sig_len, prev, prev_len = pack_beacons(beacons)
        return self.verify_records(pubkey, rounds, sigs, sig_len, prev, prev_len, mode, rlc_seed)

    def verify_records(self, pubkey, rounds, sigs, sig_len, prev, prev_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        """Fixed-stride host records (numpy, as pack_beacons builds them or
        the native bolt ingest decodes them): DGPU_REASON_* per record."""
        if len(rounds) == 0:
            return np.zeros(0, dtype=np.uint8)
        return self._records(self.ctx, self._code, pubkey, rounds, sigs, sig_len, prev, prev_len, mode, rlc_seed)

    def check_rows(self, pubkey, rows, first, count, mode=_lib.MODE_PER_ROUND, rlc_seed=None, sig_stride=96,
                   prev_stride=96, reasons=False):
        """One window of the bulk chain check in one call (dgpu_check_rows):
        `rows` is an ingest.Rows (keys, off, len, buf), the loop visits rounds
        first .. first + count - 1.  The rows are decoded and verified on the
        GPU and the faulty list is built there.  Returns (faulty_pos,
        faulty_val, left_rows): the positions (round - first) and values of
        the faulty entries in ascending position, and the indices of the rows
        that are not canonical -- the caller's to decode with
        sync.beacon_unmarshal and merge.  reasons=True appends the
        DGPU_REASON_* code per row."""
        n = len(rows.off)
        off = np.ascontiguousarray(rows.off, dtype=np.uint64)
        ln = np.ascontiguousarray(rows.len, dtype=np.uint32)
        keys = np.ascontiguousarray(rows.keys, dtype=np.uint64)
        if len(ln) != n or len(keys) != n:
            raise ValueError("rows.keys, rows.off and rows.len differ in length")
        if n and int((off + ln).max()) > rows.buf.size:
            raise ValueError("a row leaves the buffer")
        out, reason = self._rows(self.ctx, self._code, pubkey, rows.buf, off, ln, keys, sig_stride, prev_stride, mode,
                                 rlc_seed, int(first), int(count), reasons)
        return out + (reason,) if reasons else out

    def verify_segment(self, first_round, sigs, prev_sig, pubkey, mode=_lib.MODE_PER_ROUND, rlc_seed=None,
                       randomness=True, sig_len=None):
        """A linked run of rounds known by its signatures alone
        (dgpu_verify_segment; the walk of client/verify.go:118-178): round
        first_round + i carries sigs[i], its previous signature is prev_sig
        for i = 0 and sigs[i - 1] after (ignored by the unchained schemes).
        sigs: a list of bytes, or an (n, stride) uint8 array with sig_len.
        Returns (reasons, randomness): the DGPU_REASON_* codes as
        verify_records returns them, and the (n, 32) uint8 array of
        SHA-256(sigs[i]) for the rounds that verify (zeros for the others;
        client/verify.go:207), or None when randomness is False."""
        width = calls.sig_width(self._code)
        if isinstance(sigs, np.ndarray):
            if sig_len is None:
                raise ValueError("a signature array needs sig_len")
            buf = np.ascontiguousarray(sigs, dtype=np.uint8)
            lens = np.ascontiguousarray(sig_len, dtype=np.uint32)
            if buf.ndim != 2 or lens.shape != (buf.shape[0],):
                raise ValueError("sigs must be (n, stride) and sig_len (n,)")
            if buf.shape[1] < width:
                buf = np.pad(buf, ((0, 0), (0, width - buf.shape[1])))
        else:
            buf, lens = calls.pack_msgs([bytes(s or b"") for s in sigs], width)
        if buf.shape[0] == 0:
            return np.zeros(0, dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8) if randomness else None
        return self._segment(self.ctx, self._code, pubkey, first_round, buf, lens, prev_sig, mode, rlc_seed,
                             randomness)


class Verifier(RecordCalls):
    """chain.Verifier (chain/verify.go:13-20): stateless apart from the scheme;
    safe for concurrent use (the GPU context serializes).  The public key is
    passed per call, like VerifyBeacon(b, pubkey) (chain/verify.go:38); the
    context caches decoded keys, so verifiers of different chains and schemes
    can share one GPU context."""

    def __init__(self, scheme: Scheme, device=0, ctx=None):
        """ctx: a context of the caller's (default: the device's shared one)."""
        self.scheme = scheme
        self.ctx = ctx or get_context(device)
        self._code = scheme_code(scheme)

    def is_prev_sig_meaningful(self):
        """chain/verify.go:47-49"""
        return not self.scheme.decouple_prev_sig

    def digest_message(self, round_, prev_sig):
        """chain/verify.go:24-32 (computed on the GPU)."""
        return self.digest_messages([round_], [prev_sig])[0]

    def digest_messages(self, rounds, prev_sigs):
        n = len(rounds)
        r = np.asarray(rounds, dtype=np.uint64)
        stride = max([1] + [len(p or b"") for p in prev_sigs])
        prev = np.zeros((n, stride), dtype=np.uint8)
        plen = np.zeros(n, dtype=np.uint32)
        for i, p in enumerate(prev_sigs):
            if p:
                prev[i, : len(p)] = np.frombuffer(p, dtype=np.uint8)
                plen[i] = len(p)
        out = np.zeros((n, 32), dtype=np.uint8)
        lib = self.ctx.lib
        _lib.check(lib.dgpu_digest_batch(self.ctx.handle, self._code, n, _lib.ptr(r), _lib.ptr(prev), stride,
                                         _lib.ptr(plen), _lib.ptr(out)), lib)
        return [bytes(row) for row in out]

    def verify_beacons(self, beacons, pubkey, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        """Batch VerifyBeacon: returns a list of (None | VerifyError), one per beacon."""
        reasons = self.verify_reasons(beacons, pubkey, mode, rlc_seed)
        return [None if r == _lib.REASON_OK else VerifyError(b.round, int(r)) for b, r in zip(beacons, reasons)]

    def verify_rows(self, pubkey, buf, off, ln, mode=_lib.MODE_PER_ROUND, rlc_seed=None, sig_stride=96,
                    prev_stride=96):
        """Stored rows (Beacon.Marshal's bytes; row i = buf[off[i]:off[i] +
        ln[i]], as ingest.window_rows scans them), decoded and verified on the
        GPU (dgpu_verify_rows).  Returns (reasons, row_ok, rounds): the
        DGPU_REASON_* code per row, whether the row was canonical (the
        others -- reason DGPU_REASON_DECODE -- are the caller's to decode
        with sync.beacon_unmarshal), and each canonical row's Round."""
        n = len(off)
        if n == 0:
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        if int((off + ln).max()) > buf.size:
            raise ValueError("a row leaves the buffer")
        reason, ok, rounds = calls.verify_rows(self.ctx, self._code, pubkey, buf, off, ln, sig_stride, prev_stride,
                                               mode, rlc_seed)
        return reason, ok.astype(bool), rounds

    def verify_beacon(self, b: Beacon, pubkey: bytes):
        """chain/verify.go:38-45: raises VerifyError (the reference's non-nil
        error) or returns None."""
        err = self.verify_beacons([b], pubkey)[0]
        if err is not None:
            raise err


def new_verifier(scheme: Scheme, device=0):
    """chain.NewVerifier (chain/verify.go:18-20)."""
    return Verifier(scheme, device)


def verify_recovered(scheme: Scheme, pubkey, msgs, sigs, mode=_lib.MODE_PER_ROUND, rlc_seed=None, device=0,
                     ctx=None):
    """Batch key.Scheme.VerifyRecovered(pk, msg, sig) (chain/verify.go:44,
    chain/beacon/chain.go:165; kyber bls.Verify (R)) over raw messages of any
    length.  Returns the DGPU_REASON_* code per message (0 = valid).  ctx: a
    context of the caller's (default: the device's shared one)."""
    if len(msgs) == 0:
        return np.zeros(0, dtype=np.uint8)
    code = scheme_code(scheme)
    mb, ml = calls.pack_msgs(msgs)
    sb, sl = calls.pack_msgs(sigs, calls.sig_width(code))
    return calls.verify_recovered(ctx or get_context(device), code, pubkey, mb, ml, sb, sl, mode, rlc_seed)


def pack_keyed(code, keys, key_idx, msgs, sigs):
    """The host arrays of a dgpu_verify_keyed call (no device needed): the key
    table (n_keys x key_len bytes: 48 for the G2-signature schemes, 96 for the
    G1-signature schemes), the 32-bit key indices, and the fixed-stride message
    and signature records as verify_recovered packs them.  ValueError for a
    key of the wrong length or an index outside the table (the library's
    DGPU_EINVAL, raised before any call)."""
    key_len = calls.key_width(code)
    keys = [bytes(k) for k in keys]
    if not 1 <= len(keys) <= 65536:
        raise ValueError("a key table holds 1 to 65536 keys")
    if {len(k) for k in keys} != {key_len}:
        raise ValueError(f"keys of this scheme are {key_len} bytes each")
    if not (len(key_idx) == len(msgs) == len(sigs)):
        raise ValueError("key_idx, msgs and sigs differ in length")
    idx = np.ascontiguousarray(key_idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= len(keys)):
        raise ValueError("a key index lies outside the table")
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    mb, ml = calls.pack_msgs(msgs)
    sb, sl = calls.pack_msgs(sigs, calls.sig_width(code))
    return kb, key_len, idx.astype(np.uint32), mb, ml, sb, sl


def verify_keyed(scheme: Scheme, keys, key_idx, msgs, sigs, mode=_lib.MODE_PER_ROUND, rlc_seed=None, device=0,
                 ctx=None):
    """Batch bls.Verify(keys[key_idx[i]], msgs[i], sigs[i]) under a key per
    record (dgpu_verify_keyed): node identities (identity.py), or the records
    of several chains in one call.  keys: compressed public keys of the
    scheme's key group.  Returns the DGPU_REASON_* code per record (0 =
    valid); a record whose key is rejected (undecodable, outside the
    subgroup, the identity) gets REASON_KEY, whatever its signature.  ctx: a
    context of the caller's (default: the device's shared one)."""
    code = scheme_code(scheme)
    kb, key_len, idx, mb, ml, sb, sl = pack_keyed(code, keys, key_idx, msgs, sigs)
    if len(idx) == 0:
        return np.zeros(0, dtype=np.uint8)
    return calls.verify_keyed(ctx or get_context(device), code, kb, key_len, idx, mb, ml, sb, sl, mode, rlc_seed)


def hash_to_curve(msgs, scheme: Scheme = None, device=0):
    """Hash raw messages of any length to the scheme's signature group
    (compressed: 96-byte G2 under drand's DST, 48-byte G1 for the G1 schemes)."""
    from .scheme import get_scheme_by_id_with_default
    code = scheme_code(scheme or get_scheme_by_id_with_default(""))
    ctx = get_context(device)
    n = len(msgs)
    mb, ml = calls.pack_msgs(msgs)
    width = calls.sig_width(code)
    out = np.zeros(n * width, dtype=np.uint8)
    if n:
        _lib.check(ctx.lib.dgpu_hash_to_curve(ctx.handle, code, n, _lib.ptr(mb), mb.shape[1], _lib.ptr(ml),
                                              _lib.ptr(out)), ctx.lib)
    return [bytes(out[i * width:(i + 1) * width]) for i in range(n)]


def sign(secret, msgs, scheme: Scheme = None, device=0):
    """key.Scheme.Sign / AuthScheme.Sign (key/curve.go:36-39) of raw messages
    with a secret scalar (int or 32 big-endian bytes): test/tool surface."""
    from .scheme import get_scheme_by_id_with_default
    code = scheme_code(scheme or get_scheme_by_id_with_default(""))
    if not msgs:
        return []
    sk = secret if isinstance(secret, int) else bytes(secret)
    return [bytes(s) for s in calls.sign(get_context(device), code, sk, *calls.pack_msgs(msgs))]


def decode_g1_points(points, device=0):
    """Batch G1 decode (KeyGroup.Point().UnmarshalBinary, chain/convert.go:20-23):
    returns (rc list, [(x, y) ints or None])."""
    ctx = get_context(device)
    n = len(points)
    buf = np.frombuffer(b"".join(bytes(p) for p in points), dtype=np.uint8).copy()
    rc = np.zeros(n, dtype=np.int32)
    xy = np.zeros(n * 96, dtype=np.uint8)
    if n:
        _lib.check(ctx.lib.dgpu_decode_g1_points(ctx.handle, n, _lib.ptr(buf), _lib.ptr(rc), _lib.ptr(xy)), ctx.lib)
    coords = [(int.from_bytes(bytes(xy[i * 96:i * 96 + 48]), "big"), int.from_bytes(bytes(xy[i * 96 + 48:i * 96 + 96]), "big"))
              if rc[i] == 0 else None for i in range(n)]
    return rc.tolist(), coords


def _be_coords(xy, k):
    return tuple(int.from_bytes(bytes(xy[48 * j:48 * j + 48]), "big") for j in range(k))


def decode_signatures(scheme, sigs, device=0):
    """The scheme's signature decoder (the UnmarshalBinary inside bls.Verify,
    chain/verify.go:44): returns (reasons, points) with points[i] = (x, y)
    ints on G1 or ((x0, x1), (y0, y1)) on G2 for decoded records, else None."""
    ctx = get_context(device)
    code = scheme_code(scheme)
    n = len(sigs)
    g1 = code in calls.G1_SIG_CODES
    stride = max([96] + [len(s) for s in sigs])
    buf = np.zeros((max(n, 1), stride), dtype=np.uint8)
    ln = np.zeros(max(n, 1), dtype=np.uint32)
    for i, s in enumerate(sigs):
        buf[i, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        ln[i] = len(s)
    w = 96 if g1 else 192
    reason = np.zeros(max(n, 1), dtype=np.uint8)
    xy = np.zeros(max(n, 1) * w, dtype=np.uint8)
    if n:
        _lib.check(ctx.lib.dgpu_decode_signatures(ctx.handle, code, n, _lib.ptr(buf), stride, _lib.ptr(ln),
                                                  _lib.ptr(reason), _lib.ptr(xy)), ctx.lib)
    pts = []
    for i in range(n):
        if reason[i] != _lib.REASON_OK:
            pts.append(None)
            continue
        c = _be_coords(xy[i * w:(i + 1) * w], w // 48)
        pts.append(c if g1 else ((c[0], c[1]), (c[2], c[3])))
    return reason[:n].tolist(), pts


def decode_pubkey(scheme, pk, device=0):
    """The scheme's public-key decoder (chain/convert.go:20-23): the affine key
    point ((x, y) on G1, ((x0, x1), (y0, y1)) on G2); raises DrandGPUError
    (DGPU_EINVAL) when the key is rejected."""
    ctx = get_context(device)
    code = scheme_code(scheme)
    b = np.frombuffer(bytes(pk), dtype=np.uint8).copy()
    g2 = code in calls.G1_SIG_CODES
    xy = np.zeros(192, dtype=np.uint8)
    _lib.check(ctx.lib.dgpu_decode_pubkey(ctx.handle, code, _lib.ptr(b), len(pk), _lib.ptr(xy)), ctx.lib)
    c = _be_coords(xy, 4 if g2 else 2)
    return ((c[0], c[1]), (c[2], c[3])) if g2 else c


def hash_to_g2(msgs, device=0):
    """kyber G2 Hash (R) of 32-byte messages -> 96-byte compressed points (parity surface)."""
    ctx = get_context(device)
    n = len(msgs)
    m = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    out = np.zeros(n * 96, dtype=np.uint8)
    _lib.check(ctx.lib.dgpu_hash_to_g2(ctx.handle, n, _lib.ptr(m), _lib.ptr(out)), ctx.lib)
    return [bytes(out[i * 96:(i + 1) * 96]) for i in range(n)]


def hash_to_g1(msgs, scheme_code_=None, device=0):
    """Hash to G1 (RFC 9380 G1 suite) of 32-byte messages under a G1-signature
    scheme's DST -> 48-byte compressed points (parity surface)."""
    ctx = get_context(device)
    n = len(msgs)
    m = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    out = np.zeros(n * 48, dtype=np.uint8)
    code = _lib.SCHEME_UNCHAINED_G1 if scheme_code_ is None else scheme_code_
    _lib.check(ctx.lib.dgpu_hash_to_g1(ctx.handle, code, n, _lib.ptr(m), _lib.ptr(out)), ctx.lib)
    return [bytes(out[i * 48:(i + 1) * 48]) for i in range(n)]
