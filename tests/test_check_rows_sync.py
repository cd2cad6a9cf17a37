"""check_past_beacons(decode="device", replay="device") without a GPU: the
Python side of the path -- one check_rows call per window, the left rows
through beacon_unmarshal and one verify_reasons call, the merge by position,
the callbacks -- over a bolt file, with a stub verifier whose check_rows is the
rule of drand_amd/csrc/check_rows.cuh restated in numpy over the native host
decoder's records.  The yardstick is oracle/drand_ref.check_past_beacons."""
import json
import struct

import numpy as np
import pytest

from bolt_writer import write_bolt
from drand_amd.chain import Beacon
from drand_amd.sync import Cancelled, MemoryStore, beacon_marshal, check_past_beacons
from oracle import drand_ref as D

N = 40
MISSING = (5, 6, 20, 36)  # 36 = Len - 1: the last visited round has no row


def bad(sig):
    return bytes(sig[:3]) == b"BAD"


class StubRowsVerifier:
    """A beacon is valid iff its signature does not start with b"BAD"."""

    def __init__(self):
        self.check_calls, self.reason_calls, self.windows = 0, 0, []

    def verify_rows(self, *a, **k):  # (check_past_beacons asks for the attribute)
        raise AssertionError("replay='device' must not call verify_rows")

    def verify_reasons(self, beacons, pubkey, mode=0):
        self.reason_calls += 1
        return np.array([3 if bad(b.signature) else 0 for b in beacons], dtype=np.uint8)

    def check_rows(self, pubkey, rows, first, count, mode=0, rlc_seed=None):
        from drand_amd import ingest
        self.check_calls += 1
        self.windows.append((first, count))
        n = len(rows.off)
        rounds, sigs = np.zeros(n, dtype=np.uint64), np.zeros((n, 96), dtype=np.uint8)
        sig_len, prev = np.zeros(n, dtype=np.uint32), np.zeros((n, 96), dtype=np.uint8)
        prev_len, ok = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        if n:
            ingest.load().dgpu_ingest_decode(n, rows.buf.ctypes.data, rows.off.ctypes.data, rows.len.ctypes.data,
                                             rounds.ctypes.data, sigs.ctypes.data, 96, sig_len.ctypes.data,
                                             prev.ctypes.data, 96, prev_len.ctypes.data, ok.ctypes.data)
        status = np.array([3 if bad(sigs[i]) else 0 for i in range(n)], dtype=np.uint8)
        # the rule: position j of [first, first + count)
        row_of = {int(k) - first: r for r, k in enumerate(rows.keys.tolist()) if first <= int(k) < first + count}
        pos, val, left = [], [], []
        for j in range(count):
            r = row_of.get(j)
            if r is None:
                pos.append(j), val.append(first + j)
            elif not ok[r]:
                left.append(r)
            elif status[r]:
                pos.append(j), val.append(int(rounds[r]))
        return np.array(pos, dtype=np.uint64), np.array(val, dtype=np.uint64), np.array(left, dtype=np.uint64)


def spaced(b):
    return json.dumps({"PreviousSig": b.previous_sig.hex(), "Round": b.round, "Signature": b.signature.hex()}).encode()


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """(BoltStore, the oracle's table): rounds 0 .. 40 with rows missing, an
    undecodable row, a valid and an invalid beacon stored as JSON with
    whitespace, failing rows, one of them with Round != key."""
    from drand_amd.boltstore import BoltStore
    st = MemoryStore()
    table = {0: (0, b"", b"genesis")}
    st.put(Beacon(b"", 0, b"genesis"))
    for r in range(1, N + 1):
        if r in MISSING:
            continue
        b = Beacon(b"p%d" % r, r, (b"BAD" if r in (3, 17, 30) else b"ok") + bytes([r]))
        if r == 17:
            b.round = 1017  # a failing row whose stored Round is not its key
        raw = beacon_marshal(b)
        if r in (12, 13):  # not canonical: the full decoder's rows; 13 fails verification
            b.signature = (b"BAD" if r == 13 else b"ok") + bytes([r])
            raw = spaced(b)
        table[r] = (b.round, b.previous_sig, b.signature)
        if r == 9:
            raw, table[r] = b"not json", None  # Get's unmarshal error: the round is faulty
        st.put_raw(r, raw)
    p = tmp_path_factory.mktemp("check_rows_sync") / "drand.db"
    write_bolt(p, dict(st._kv))
    bs = BoltStore(p)
    yield bs, table
    bs.close()


@pytest.mark.parametrize("window", [16, 7, None])
def test_replay_device_matches_the_oracle(stores, window):
    bs, table = stores
    length = bs.len()
    assert length == N + 1 - len(MISSING) and length - 1 in MISSING
    for up_to in (0, 1, 15, length - 1, length + 5):
        exp, progress = D.check_past_beacons(table, up_to, lambda b: not bad(b[2]))
        v = StubRowsVerifier()
        calls = []
        got = check_past_beacons(bs, v, b"pk", up_to, cb=lambda i, u: calls.append((i, u)), window=window,
                                 decode="device", replay="device")
        assert got == exp and calls == progress, (up_to, got, exp)
        v2 = StubRowsVerifier()
        assert check_past_beacons(bs, v2, b"pk", up_to, window=window, decode="device", replay="device") == exp
        visited = len(progress)
        assert v.check_calls == v2.check_calls == (1 if window is None else -(-visited // window))
        assert v.windows[0][0] == 1 and sum(c for _, c in v.windows) == visited
        # one verify_reasons call per window that holds a decodable left row
        assert v.reason_calls <= v.check_calls
    full, _ = D.check_past_beacons(table, length + 5, lambda b: not bad(b[2]))
    assert full == [3, 5, 6, 9, 13, 1017, 20, 30, 36]


def test_replay_device_arguments_and_cancellation(stores):
    bs, _ = stores
    v = StubRowsVerifier()
    with pytest.raises(ValueError):
        check_past_beacons(bs, v, b"pk", 10, decode="host", replay="device")
    with pytest.raises(ValueError):
        check_past_beacons(bs, v, b"pk", 10, decode="device", replay="gpu")

    class NoCheckRows:
        verify_rows = verify_reasons = None
    with pytest.raises(ValueError):
        check_past_beacons(bs, NoCheckRows(), b"pk", 10, decode="device", replay="device")
    seen = []
    with pytest.raises(Cancelled):
        check_past_beacons(bs, v, b"pk", 30, cb=lambda i, u: seen.append(i), cancelled=lambda: len(seen) >= 4,
                           window=16, decode="device", replay="device")
    assert seen == [1, 2, 3, 4]
    # the default replay leaves the existing device-decode path as it was: no check_rows call
    class RowsOnly(StubRowsVerifier):
        def verify_rows(self, pubkey, buf, off, ln, mode=0):
            n = len(off)
            return np.zeros(n, dtype=np.uint8), np.ones(n, dtype=bool), np.arange(n, dtype=np.uint64)
    r = RowsOnly()
    check_past_beacons(bs, r, b"pk", 3, decode="device")
    assert r.check_calls == 0
