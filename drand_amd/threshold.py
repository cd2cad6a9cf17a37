"""Threshold recovery (drand's aggregator path) on the GPU through the C-ABI.

Mirrors (names, argument meaning, error behaviour):
  key.Scheme.IndexOf(partial)                    kyber tbls.SigShare.Index (R); node.go:119
  key.Scheme.Recover(pub, msg, sigs, t, n)       kyber tbls.Recover (R); chain/beacon/chain.go:160
and the batch form an aggregator or a catch-up recomputation needs:
  ThresholdGroup.recover_batch(msgs, partials)   one GPU call for many rounds

A share.PubPoly is represented by its t compressed commitments (key/keys.go
DistPublic.Coefficients): 48-byte G1 points for the G2-signature schemes,
96-byte G2 points for the G1-signature schemes (bls-unchained-on-g1,
bls-unchained-g1-rfc9380), whose partials are BE16(index) || 48-byte G1
signature and whose recovered signatures are 48 bytes.  No CPU fallback: the
work runs in libdrand_gpu.so (dgpu_set_group_scheme / dgpu_recover_batch).
Any threshold 1 <= t <= 1024 (DGPU_MAX_THRESHOLD) is accepted: above 32 the
group is installed with dgpu_set_group_wide (calls.set_group) and the library
takes its wide recovery path; above 1024 the library's error is raised.
"""
import struct
import threading

import numpy as np

from . import _lib, calls
from .calls import G1_SIG_CODES as _G1_SIG_CODES, sig_width as sig_bytes  # noqa: F401  (sig_bytes: the older name)
from .chain import get_context
from .scheme import Scheme, get_scheme_by_id_with_default, scheme_code


def group_scheme_code(commits, scheme=None):
    """The scheme code a group of these commitments installs under: `scheme`
    is a scheme name, a Scheme or a code; None means the default G2-signature
    group and needs 48-byte commitments.  ValueError if the commitments'
    length does not fit the scheme's key group (96 bytes for the G1-signature
    schemes, 48 otherwise)."""
    if scheme is None:
        code = _lib.SCHEME_CHAINED
    elif isinstance(scheme, Scheme):
        code = scheme_code(scheme)
    elif isinstance(scheme, str):
        code = scheme_code(get_scheme_by_id_with_default(scheme))
    else:
        code = int(scheme)
        if code not in (_lib.SCHEME_CHAINED, _lib.SCHEME_UNCHAINED) + _G1_SIG_CODES:
            raise ValueError(f"scheme code {code} is not valid")
    want = calls.key_width(code)
    lens = {len(c) for c in commits}
    if lens != {want}:
        if scheme is None and lens == {96}:
            raise ValueError("96-byte (G2) commitments need a G1-signature scheme")
        raise ValueError(f"commitments of lengths {sorted(lens)} do not fit the scheme ({want} bytes each)")
    return code


class RecoverError(Exception):
    """The reference's Recover error ("not enough good public shares to
    reconstruct secret commitment")."""


def index_of(partial):
    """key.Scheme.IndexOf: BE16 of the first two bytes; error (-1) if shorter."""
    if len(partial) < 2:
        return -1
    return struct.unpack(">H", partial[:2])[0]


def pack_partials(msgs, partials, scheme=_lib.SCHEME_CHAINED):
    """Fixed-stride partial records of the C-ABI: (msgs (nr*32,), partials
    (nr, m, stride), partial_len (nr, m), m, stride); empty slots have length 0.
    The stride is at least the scheme's partial length (2 + signature bytes)."""
    nr = len(msgs)
    m = max(1, max(len(p) for p in partials))
    stride = max([2 + sig_bytes(scheme)] + [len(s) for p in partials for s in p])
    buf = np.zeros((nr, m, stride), dtype=np.uint8)
    plen = np.zeros((nr, m), dtype=np.uint32)
    for r, plist in enumerate(partials):
        for j, s in enumerate(plist):
            plen[r, j] = len(s)
            if s:
                buf[r, j, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    mb = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    if mb.size != 32 * nr:
        raise ValueError("messages must be 32 bytes (DigestMessage output)")
    return mb, buf, plen, m, stride


def unpack_recovered(out, ok, pv, partials, m, sig_len=96):
    nr = len(partials)
    okb = np.unpackbits(ok, bitorder="little")[:nr]
    sigs = [bytes(out[sig_len * r:sig_len * (r + 1)]) if okb[r] else None for r in range(nr)]
    if pv is None:
        return sigs, None
    valid = [[bool(pv[r * m + j]) for j in range(len(partials[r]))] for r in range(nr)]
    return sigs, valid


class ThresholdGroup:
    """A group's share.PubPoly installed on one GPU context.  A context holds
    one group at a time and calls.set_group records which on the context
    object, so groups that share a context take turns."""

    _lock = threading.Lock()

    def __init__(self, commits, n, device=0, scheme=None, ctx=None):
        """scheme: None (48-byte G1 commitments, G2 signatures, as always), or
        a scheme name / Scheme / code; 96-byte G2 commitments require one of
        the G1-signature schemes.  A mismatch raises ValueError before any
        library call.  ctx: a context of the caller's (default: the device's
        shared one)."""
        self.commits = [bytes(c) for c in commits]
        self.scheme_code = group_scheme_code(self.commits, scheme)
        self.sig_len = sig_bytes(self.scheme_code)
        self.t = len(self.commits)
        self.n = n
        self.ctx = ctx or get_context(device)
        with ThresholdGroup._lock:
            self._key = calls.set_group(self.ctx, self.scheme_code, self.t, n, self.commits)

    def _install(self):
        if getattr(self.ctx, "installed_group", None) != self._key:
            calls.set_group(self.ctx, self.scheme_code, self.t, self.n, self.commits)

    def recover_batch(self, msgs, partials, statuses=True):
        """msgs: list of 32-byte messages (DigestMessage of each round);
        partials: list (per round) of lists of partial signatures (bytes).
        Returns (sigs, valid): sigs[r] = recovered signature (96 bytes; 48
        for a G1-signature group) or None
        (the reference's error), valid[r][j] = partial j verified.  With
        statuses=False valid is None and the library verifies each round's
        candidates with one batched pairing (recover.cuh)."""
        if len(msgs) == 0:
            return [], []
        mb, buf, plen, m, stride = pack_partials(msgs, partials, self.scheme_code)
        with ThresholdGroup._lock:
            self._install()
            out, ok, pv = calls.recover_batch(self.ctx, mb, buf, plen, self.sig_len, statuses)
        return unpack_recovered(out, ok, pv, partials, m, self.sig_len)

    def verify_partials(self, msgs, partials, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        """key.Scheme.VerifyPartial of every partial (chain/beacon/node.go:
        117-125) without recovering: msgs and partials as recover_batch takes
        them.  Returns reasons[r][j], the DGPU_REASON_* code of partial j of
        round r alone (0 = it verifies under PubPoly.Eval(its index); an empty
        or mis-sized partial is DGPU_REASON_DECODE).  No "stop after t" and no
        duplicate rule apply."""
        nr = len(msgs)
        if nr == 0:
            return []
        mb, buf, plen, m, stride = pack_partials(msgs, partials, self.scheme_code)
        with ThresholdGroup._lock:
            self._install()
            reason = calls.verify_partials(self.ctx, mb, buf, plen, mode, rlc_seed)
        return [[int(reason[r * m + j]) for j in range(len(partials[r]))] for r in range(nr)]

    def recover(self, msg, sigs):
        """key.Scheme.Recover(pub, msg, sigs, t, n): the recovered signature
        (96 bytes, 48 for a G1-signature group), or RecoverError."""
        out, _ = self.recover_batch([msg], [list(sigs)], statuses=False)
        if out[0] is None:
            raise RecoverError("share: not enough good public shares to reconstruct secret commitment")
        return out[0]
