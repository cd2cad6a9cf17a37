"""Multi-GPU verification through the C ABI (dgpu_multi_open /
dgpu_verify_multi, include/drand_gpu.h): one process drives every GPU of a
node, as a Go caller of the crypto/gpu package would.
Rounds shard contiguously across the devices; RCCL over xGMI gathers only
the per-device verdict bitmaps (and, in RLC mode, the per-device RLC roots,
checked once).  Verdicts equal chain.Verifier's on the same beacons.

The one-process-per-GPU form (torch.distributed ranks, bench.py) lives in
drand_amd/dist.py; both shard with the same contiguous rule."""
import numpy as np

from . import _lib
from .chain import Verifier, check_rows_with, pack_beacons, rlc_seed_for, verify_segment_with
from .scheme import Scheme, scheme_code
from .threshold import group_scheme_code, pack_partials, sig_bytes, unpack_recovered


class MultiVerifier:
    """chain.Verifier's batch surface over several GPUs (one dgpu_multi handle)."""

    def __init__(self, scheme: Scheme, devices=None, mctx=None):
        self.scheme = scheme
        self._code = scheme_code(scheme)
        self.mctx = mctx if mctx is not None else _lib.MultiContext(devices)

    def close(self):
        self.mctx.close()

    def verify_reasons(self, beacons, pubkey, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        n = len(beacons)
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        rounds, sigs, sig_len, prev, prev_len = pack_beacons(beacons)
        return self.verify_records(pubkey, rounds, sigs, sig_len, prev, prev_len, mode, rlc_seed)

    def verify_records(self, pubkey, rounds, sigs, sig_len, prev, prev_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None):
        """Fixed-stride host records (numpy, as chain.pack_beacons builds)."""
        n = len(rounds)
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        reason = np.zeros(n, dtype=np.uint8)
        pk = np.frombuffer(bytes(pubkey), dtype=np.uint8).copy()
        lib = self.mctx.lib
        _lib.check(lib.dgpu_verify_multi(self.mctx.handle, self._code, _lib.ptr(pk), pk.size, n, _lib.ptr(rounds),
                                         _lib.ptr(sigs), sigs.shape[1], _lib.ptr(sig_len), _lib.ptr(prev),
                                         prev.shape[1], _lib.ptr(prev_len), mode, rlc_seed_for(mode, rlc_seed),
                                         _lib.ptr(bits), _lib.ptr(reason)))
        valid = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
        if not np.array_equal(valid, reason == _lib.REASON_OK):
            raise _lib.DrandGPUError(_lib.DGPU_EINVAL, "verdict bitmap and reasons disagree")
        return reason

    def verify_segment(self, first_round, sigs, prev_sig, pubkey, mode=_lib.MODE_PER_ROUND, rlc_seed=None,
                       randomness=True, sig_len=None):
        """chain.Verifier.verify_segment over the handle's GPUs
        (dgpu_verify_segment_multi): the same arguments, the same
        (reasons, randomness) result.  The rounds shard contiguously; a later
        shard's first round takes the record before the shard as its halo."""
        lib = self.mctx.lib
        return verify_segment_with(lambda *a: lib.dgpu_verify_segment_multi(self.mctx.handle, self._code, *a), lib,
                                   self._code, first_round, sigs, prev_sig, pubkey, mode, rlc_seed, randomness,
                                   sig_len)


    def _shard_verifiers(self):
        """One chain.Verifier per device of the handle, over the handle's own
        contexts (dgpu_multi_context; the handle keeps owning them)."""
        if getattr(self, "_shards", None) is None:
            import ctypes
            self._shards = []
            for k in range(len(self.mctx.devices)):
                h = ctypes.c_void_p()
                _lib.check(self.mctx.lib.dgpu_multi_context(self.mctx.handle, k, ctypes.byref(h)), self.mctx.lib)
                v = Verifier.__new__(Verifier)
                v.scheme, v._code, v.ctx = self.scheme, self._code, _BorrowedContext(self.mctx.lib, h)
                self._shards.append(v)
        return self._shards

    def verify_rows(self, pubkey, buf, off, ln, mode=_lib.MODE_PER_ROUND, rlc_seed=None, sig_stride=96,
                    prev_stride=96):
        """chain.Verifier.verify_rows over the handle's GPUs: the same
        arguments and the same (reasons, row_ok, rounds) result.  The rows
        shard on the host by dgpu_shard_range and each shard is one
        dgpu_verify_rows call on its device's context, side by side (RLC
        mode: each shard checks its own combination)."""
        from concurrent.futures import ThreadPoolExecutor
        n = len(off)
        shards = self._shard_verifiers()
        cuts = [_lib.shard_range(n, len(shards), k) for k in range(len(shards))]
        seed = rlc_seed_for(mode, rlc_seed)

        def part(k):
            lo, hi = cuts[k]
            return shards[k].verify_rows(pubkey, buf, off[lo:hi], ln[lo:hi], mode, seed, sig_stride, prev_stride)
        with ThreadPoolExecutor(len(shards)) as ex:
            parts = list(ex.map(part, range(len(shards))))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

    def check_rows(self, pubkey, rows, first, count, mode=_lib.MODE_PER_ROUND, rlc_seed=None, sig_stride=96,
                   prev_stride=96, reasons=False):
        """chain.Verifier.check_rows over the handle's GPUs
        (dgpu_check_rows_multi): the same arguments, the same lists."""
        lib = self.mctx.lib
        return check_rows_with(lambda *a: lib.dgpu_check_rows_multi(self.mctx.handle, self._code, *a), lib, pubkey,
                               rows, first, count, mode, rlc_seed, sig_stride, prev_stride, reasons)


class _BorrowedContext:
    """A context of a dgpu_multi handle as chain.Verifier holds one: the
    library and the handle, not owned."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle


class MultiThresholdGroup:
    """ThresholdGroup's batch recovery over several GPUs (dgpu_multi_set_group
    + dgpu_recover_multi): rounds shard contiguously across the devices."""

    def __init__(self, commits, n, devices=None, mctx=None, scheme=None):
        """scheme as ThresholdGroup's: None for 48-byte G1 commitments, a
        G1-signature scheme (name, Scheme or code) for 96-byte G2 ones."""
        self.commits = [bytes(c) for c in commits]
        self.scheme_code = group_scheme_code(self.commits, scheme)
        self.sig_len = sig_bytes(self.scheme_code)
        self.t, self.n = len(self.commits), n
        self.mctx = mctx if mctx is not None else _lib.MultiContext(devices)
        buf = np.frombuffer(b"".join(self.commits), dtype=np.uint8).copy()
        if self.sig_len == 96:
            _lib.check(self.mctx.lib.dgpu_multi_set_group(self.mctx.handle, self.t, n, _lib.ptr(buf)))
        else:
            _lib.check(self.mctx.lib.dgpu_multi_set_group_scheme(self.mctx.handle, self.scheme_code, self.t, n,
                                                                 _lib.ptr(buf), len(self.commits[0])))

    def close(self):
        self.mctx.close()

    def recover_batch(self, msgs, partials, statuses=True):
        """As ThresholdGroup.recover_batch: (sigs or None per round, per-partial validity or None)."""
        nr = len(msgs)
        if nr == 0:
            return [], []
        mb, buf, plen, m, stride = pack_partials(msgs, partials, self.scheme_code)
        return self.recover_records(mb, buf, plen, partials, statuses)

    def recover_records(self, mb, buf, plen, partials=None, statuses=False):
        nr, m, stride = buf.shape
        out = np.zeros(nr * self.sig_len, dtype=np.uint8)
        ok = np.zeros((nr + 7) // 8, dtype=np.uint8)
        pv = np.zeros(nr * m, dtype=np.uint8) if statuses else None
        _lib.check(self.mctx.lib.dgpu_recover_multi(self.mctx.handle, nr, _lib.ptr(mb), m, _lib.ptr(buf), stride,
                                                    _lib.ptr(plen), _lib.ptr(out), _lib.ptr(ok), _lib.ptr(pv)))
        if partials is None:
            partials = [[b"x"] * m for _ in range(nr)]
        return unpack_recovered(out, ok, pv, partials, m, self.sig_len)
