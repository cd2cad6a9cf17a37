"""Multi-GPU verification through the C ABI (dgpu_multi_open /
dgpu_verify_multi, include/drand_gpu.h): one process drives every GPU of a
node, as a Go caller of the crypto/gpu package would.
Rounds shard contiguously across the devices; RCCL over xGMI gathers only
the per-device verdict bitmaps (and, in RLC mode, the per-device RLC roots,
checked once).  Verdicts equal chain.Verifier's on the same beacons.

The one-process-per-GPU form (torch.distributed ranks, bench.py) lives in
drand_amd/dist.py; both shard with the same contiguous rule."""
import numpy as np

from . import _lib, calls
from .chain import RecordCalls, Verifier
from .scheme import Scheme, scheme_code
from .threshold import group_scheme_code, pack_partials, unpack_recovered


class MultiVerifier(RecordCalls):
    """chain.Verifier's batch surface over several GPUs (one dgpu_multi
    handle): verify_reasons, verify_records, verify_segment and check_rows are
    chain.Verifier's, under dgpu_verify_multi, dgpu_verify_segment_multi (a
    later shard's first round takes the record before the shard as its halo)
    and dgpu_check_rows_multi."""

    _records = staticmethod(calls.verify_multi)
    _segment = staticmethod(calls.verify_segment_multi)
    _rows = staticmethod(calls.check_rows_multi)

    def __init__(self, scheme: Scheme, devices=None, mctx=None):
        self.scheme = scheme
        self._code = scheme_code(scheme)
        self.mctx = self.ctx = mctx if mctx is not None else _lib.MultiContext(devices)

    def close(self):
        self.mctx.close()

    def _shard_verifiers(self):
        """One chain.Verifier per device of the handle, over the handle's own
        contexts (dgpu_multi_context; the handle keeps owning them)."""
        if getattr(self, "_shards", None) is None:
            self._shards = [Verifier(self.scheme, ctx=calls.multi_context(self.mctx, k))
                            for k in range(len(self.mctx.devices))]
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
        seed = calls.rlc_seed_for(mode, rlc_seed)

        def part(k):
            lo, hi = cuts[k]
            return shards[k].verify_rows(pubkey, buf, off[lo:hi], ln[lo:hi], mode, seed, sig_stride, prev_stride)
        with ThreadPoolExecutor(len(shards)) as ex:
            parts = list(ex.map(part, range(len(shards))))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


class MultiThresholdGroup:
    """ThresholdGroup's batch recovery over several GPUs (dgpu_multi_set_group
    + dgpu_recover_multi): rounds shard contiguously across the devices."""

    def __init__(self, commits, n, devices=None, mctx=None, scheme=None):
        """scheme as ThresholdGroup's: None for 48-byte G1 commitments, a
        G1-signature scheme (name, Scheme or code) for 96-byte G2 ones."""
        self.commits = [bytes(c) for c in commits]
        self.scheme_code = group_scheme_code(self.commits, scheme)
        self.sig_len = calls.sig_width(self.scheme_code)
        self.t, self.n = len(self.commits), n
        self.mctx = mctx if mctx is not None else _lib.MultiContext(devices)
        calls.multi_set_group(self.mctx, self.scheme_code, self.t, n, self.commits)

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
        m = buf.shape[1]
        out, ok, pv = calls.recover_multi(self.mctx, mb, buf, plen, self.sig_len, statuses)
        if partials is None:
            partials = [[b"x"] * m for _ in range(len(buf))]
        return unpack_recovered(out, ok, pv, partials, m, self.sig_len)
