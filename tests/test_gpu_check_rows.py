"""The check-chain loop's faulty list built on the GPU
(dgpu_faulty_rounds_device, dgpu_check_rows,
check_past_beacons(decode="device", replay="device")).

The yardsticks: for the device stage, the rule of
drand_amd/csrc/check_rows.cuh restated in numpy over synthetic arrays; for
dgpu_check_rows, that rule applied to dgpu_verify_rows' outputs on the same
rows and a list written out by hand; for the loop, replay="host" with either
decoder."""
import contextlib
import json
import os

import numpy as np
import pytest

from bolt_writer import write_bolt
from conftest import load_golden, open_ctx
from ingest_rows_corpus import marshal, pack

pytestmark = pytest.mark.gpu
BLOCK = 256  # CHECK_BLOCK: positions per block, block counts per pass of the scan (check_rows.cuh)
GUARD = 64


def rule(first, count, keys, ok, rounds, status):
    """(faulty_pos, faulty_val, left_rows) of the visited range."""
    pos = keys.astype(np.int64) - first if len(keys) else np.zeros(0, dtype=np.int64)
    inside = (keys >= first) & (keys - np.uint64(first) < count) if len(keys) else np.zeros(0, dtype=bool)
    row = np.full(count, -1, dtype=np.int64)
    row[pos[inside]] = np.nonzero(inside)[0]
    has = row >= 0
    r = np.where(has, row, 0)
    if len(keys) == 0:
        ok, rounds, status = np.ones(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
    left = has & (ok[r] == 0)
    fail = has & (ok[r] != 0) & (status[r] != 0)
    faulty = ~has | fail
    val = np.where(has, rounds[r], np.uint64(first) + np.arange(count, dtype=np.uint64))
    return np.nonzero(faulty)[0].astype(np.uint64), val[faulty].astype(np.uint64), row[left].astype(np.uint64)


def device_stage(ctx, first, count, keys, ok, rounds, status, fcap, lcap):
    """dgpu_faulty_rounds_device over device copies; the lists carry guard
    bytes behind their caps.  Returns (pos, val, left, totals)."""
    import torch
    from drand_amd import _lib

    def dev(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda() if len(a) else None
    d_keys, d_rounds = dev(keys, np.int64), dev(rounds, np.int64)
    d_ok, d_status = dev(ok, np.uint8), dev(status, np.uint8)
    out = {k: torch.full((8 * cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
           for k, cap in (("pos", fcap), ("val", fcap), ("left", lcap), ("counts", 2))}
    _lib.check(ctx.lib.dgpu_faulty_rounds_device(
        ctx.handle, first, count, len(keys), _lib.ptr(d_keys), _lib.ptr(d_ok), _lib.ptr(d_rounds), _lib.ptr(d_status),
        _lib.ptr(out["pos"]), _lib.ptr(out["val"]), fcap, _lib.ptr(out["left"]), lcap, _lib.ptr(out["counts"]), None),
        ctx.lib)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert (v[-GUARD:] == 0xA5).all(), f"{k}: written past its cap"
    totals = host["counts"][:16].view(np.uint64)
    nf, nl = min(int(totals[0]), fcap), min(int(totals[1]), lcap)
    pos, val, left = (host[k][:-GUARD].view(np.uint64) for k in ("pos", "val", "left"))
    # entries at or past the totals stay untouched too
    assert (host["pos"][8 * nf:] == 0xA5).all() and (host["val"][8 * nf:] == 0xA5).all()
    assert (host["left"][8 * nl:] == 0xA5).all()
    return pos[:nf], val[:nf], left[:nl], totals


def window(first, count, missing, left=(), fail=(), moved=(), outside=True):
    """Rows for every position of [first, first + count) not in `missing`
    (positions); rows at `left` are not canonical, rows at `fail` fail, rows
    at `moved` store another Round; one key on either side of the range."""
    present = np.setdiff1d(np.arange(count), np.asarray(missing, dtype=np.int64))
    keys = (first + present).astype(np.uint64)
    ok, status, rounds = np.ones(len(keys), dtype=np.uint8), np.zeros(len(keys), dtype=np.uint8), keys.copy()
    at = {int(p): i for i, p in enumerate(present.tolist())}
    for p in left:
        ok[at[p]] = 0
        rounds[at[p]] = 0
    for p in fail:
        status[at[p]] = 1 + p % 4
    for p in moved:
        rounds[at[p]] += 1000
    if outside:  # keys outside the range take no part, whatever their rows say
        keys = np.concatenate([[first - 1], keys, [first + count + 3]]).astype(np.uint64)
        ok = np.concatenate([[1], ok, [0]]).astype(np.uint8)
        status = np.concatenate([[3], status, [3]]).astype(np.uint8)
        rounds = np.concatenate([[7], rounds, [9]]).astype(np.uint64)
    return keys, ok, rounds, status


# both sides of the wave (64), of the block (256), two blocks + 1, and one
# count above what a single pass of the block-sum scan covers (256 blocks)
@pytest.mark.parametrize("count", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, BLOCK * BLOCK + 1])
def test_device_stage_equals_the_rule(gpu_ctx, count):
    first = 1000
    every = np.arange(count)
    inner = every[BLOCK // 2:count - 1]  # every interior block whole once count > 2 blocks; faults at 0 and count - 1
    rng = np.random.default_rng(count)
    mixed_missing = every[rng.random(count) < 0.2]
    rest = np.setdiff1d(every, mixed_missing)
    patterns = {
        "no fault": window(first, count, []),
        "n = 0": tuple(np.zeros(0, dtype=t) for t in (np.uint64, np.uint8, np.uint64, np.uint8)),
        "every position faulty": window(first, count, [], fail=every, outside=False),
        "every row missing but the first": window(first, count, every[1:]),
        "first and last": window(first, count, [], fail={0, count - 1}),
        "a run of missing rounds over interior blocks": window(first, count, inner, fail={0, count - 1},
                                                               left=[1] if count > 2 and 1 not in inner else []),
        "alternating": window(first, count, [], fail=every[::2]),
        "mixed": window(first, count, mixed_missing, left=rest[::7], fail=rest[1::3], moved=rest[::5]),
    }
    for name, (keys, ok, rounds, status) in patterns.items():
        want = rule(first, count, keys, ok, rounds, status)
        pos, val, left, totals = device_stage(gpu_ctx, first, count, keys, ok, rounds, status, count, max(len(keys), 1))
        assert totals.tolist() == [len(want[0]), len(want[2])], (name, totals)
        assert np.array_equal(pos, want[0]) and np.array_equal(val, want[1]), name
        assert np.array_equal(left, want[2]), name
        # truncation: caps below the totals, the totals still exact
        fcap, lcap = len(want[0]) // 2, len(want[2]) // 3
        pos, val, left, totals = device_stage(gpu_ctx, first, count, keys, ok, rounds, status, fcap, lcap)
        assert totals.tolist() == [len(want[0]), len(want[2])], (name, "truncated")
        assert np.array_equal(pos, want[0][:fcap]) and np.array_equal(val, want[1][:fcap]), (name, "truncated")
        assert np.array_equal(left, want[2][:lcap]), (name, "truncated")
    if count > 2 * BLOCK:
        assert inner[0] < BLOCK and inner[-1] == (count - 1) // BLOCK * BLOCK - 1  # the run covers whole blocks
    # Round != key really is reported: the mixed pattern's values are not all keys
    keys, ok, rounds, status = patterns["mixed"]
    w = rule(first, count, keys, ok, rounds, status)
    assert count < 64 or (w[1] != first + w[0]).any()


def test_device_stage_empty_range_and_bad_arguments(gpu_ctx):
    from drand_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    _lib.check(lib.dgpu_faulty_rounds_device(h, 5, 0, 0, None, None, None, None, None, None, 0, None, 0, None, None), lib)
    assert lib.dgpu_faulty_rounds_device(h, 2 ** 64 - 3, 4, 0, None, None, None, None, None, None, 0, None, 0, None,
                                         None) == _lib.DGPU_EINVAL  # first + count overflows
    assert lib.dgpu_faulty_rounds_device(h, 1, 4, 0, None, None, None, None, None, None, 0, None, 0, None,
                                         None) == _lib.DGPU_EINVAL  # no count buffer
    keys, ok, rounds, status = window(10, 5, [2], outside=False)
    pos, val, left, totals = device_stage(gpu_ctx, 10, 5, keys, ok, rounds, status, 5, 5)
    assert (pos.tolist(), val.tolist(), left.tolist()) == ([2], [12], [])
    # duplicate and descending keys: which row wins is unspecified, the totals of the missing rounds are not
    keys = np.array([12, 12, 11, 2 ** 64 - 1, 0], dtype=np.uint64)
    one, zero = np.ones(5, dtype=np.uint8), np.zeros(5, dtype=np.uint8)
    pos, val, left, totals = device_stage(gpu_ctx, 10, 5, keys, one, keys, zero, 5, 5)
    assert pos.tolist() == [0, 3, 4] and val.tolist() == [10, 13, 14] and totals.tolist() == [3, 0]


# ---------------------------------------------------------------- dgpu_check_rows
def verify_rows(ctx, code, pk, buf, off, ln, ss, ps, mode, seed):
    from drand_amd import calls
    reason, ok, rounds = calls.verify_rows(ctx, code, pk, buf, off, ln, ss, ps, mode, seed, fill=0xEE)
    return rounds, ok, reason


def check_rows(ctx, code, pk, buf, off, ln, keys, ss, ps, mode, seed, first, count, fcap=None, lcap=None, reason=False,
               call=None):
    """dgpu_check_rows (or `call`, the _multi form with its handle bound) with
    guard words behind both lists: (pos, val, left, totals[, reason])."""
    from drand_amd import _lib
    n = len(off)
    fcap = count if fcap is None else fcap
    lcap = n if lcap is None else lcap
    G = np.uint64(0xA5A5A5A5A5A5A5A5)
    pos, val, left = np.full(fcap + 2, G), np.full(fcap + 2, G), np.full(lcap + 2, G)
    nf, nl = np.full(1, G), np.full(1, G)
    rs = np.full(n + 2, 0xEE, dtype=np.uint8) if reason else None
    fn = call or (lambda *a: ctx.lib.dgpu_check_rows(ctx.handle, *a))
    rc = fn(code, _lib.ptr(pk), pk.size, n, _lib.ptr(buf), _lib.ptr(off), _lib.ptr(ln), _lib.ptr(keys), ss, ps, mode,
            seed, first, count, _lib.ptr(pos), _lib.ptr(val), fcap, _lib.ptr(nf), _lib.ptr(left), lcap, _lib.ptr(nl),
            _lib.ptr(rs))
    _lib.check(rc, ctx.lib)
    assert (pos[fcap:] == G).all() and (val[fcap:] == G).all() and (left[lcap:] == G).all()
    a, b = min(int(nf[0]), fcap), min(int(nl[0]), lcap)
    assert (pos[a:] == G).all() and (left[b:] == G).all()
    out = (pos[:a], val[:a], left[:b], [int(nf[0]), int(nl[0])])
    if reason:
        assert (rs[n:] == 0xEE).all()
        out += (rs[:n],)
    return out


def planted_store():
    """The bolt file of test_check_past_beacons_device_decode_equals_host_decode,
    rebuilt: 200 chained rounds with two rows missing, a valid and a corrupted
    beacon stored as JSON with whitespace, an undecodable row, corrupted
    signatures, a signature and a previous signature above the stride, a row
    whose Round differs from its key, an upper-case row.  Returns (MemoryStore,
    chain, [(visited round, faulty value)])."""
    from drand_amd import _lib
    from drand_amd.chain import Beacon
    from drand_amd.sync import MemoryStore, beacon_marshal
    from drand_amd.synth import make_chain
    n = 200
    c = make_chain(77, n, _lib.SCHEME_CHAINED, seg_len=8)
    st = MemoryStore()
    st.put(Beacon(b"", 0, c.genesis))

    def beacon(i, round_=None, sig=None, prev=None):  # chain item i = round i + 1
        return Beacon(bytes(c.prev[i, :c.prev_len[i]]) if prev is None else prev,
                      int(c.rounds[i]) if round_ is None else round_, bytes(c.sigs[i, :c.sig_len[i]]) if sig is None else sig)

    def spaced(b):
        return json.dumps({"PreviousSig": b.previous_sig.hex(), "Round": b.round, "Signature": b.signature.hex()}).encode()

    def flipped(i):
        s = bytearray(c.sigs[i].tobytes())
        s[40] ^= 4
        return bytes(s)
    for i in range(n):
        st.put(beacon(i))
    for r in (17, 150):
        st.delete(r)
    st.put_raw(40, spaced(beacon(39)))
    st.put_raw(41, spaced(beacon(40, sig=flipped(40))))
    st.put_raw(60, b"not json")
    st.put_raw(80, beacon_marshal(beacon(79, sig=flipped(79))))
    st.put_raw(81, beacon_marshal(beacon(80, sig=b"")))
    st.put_raw(100, beacon_marshal(beacon(99, round_=107)))
    st.put_raw(120, beacon_marshal(beacon(119, sig=bytes(c.sigs[119]) + b"\x01")))
    st.put_raw(130, beacon_marshal(beacon(129, prev=bytes(c.prev[129]) + b"\x01\x02\x03\x04")))
    st.put_raw(190, beacon_marshal(beacon(189)).upper().replace(b"PREVIOUSSIG", b"PreviousSig").replace(
        b"ROUND", b"Round").replace(b"SIGNATURE", b"Signature"))
    want = [(17, 17), (41, 41), (60, 60), (80, 80), (81, 81), (100, 107), (120, 120), (130, 130), (150, 150)]
    return st, c, want


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    from drand_amd.boltstore import BoltStore
    st, c, want = planted_store()
    p = tmp_path_factory.mktemp("check_rows") / "drand.db"
    write_bolt(p, dict(st._kv))
    bs = BoltStore(p)
    yield bs, c, want
    bs.close()


@pytest.mark.parametrize("mode", ["MODE_PER_ROUND", "MODE_RLC"])
def test_check_rows_on_the_planted_bolt_file(planted, gpu_ctx, mode):
    """One window over the whole range, then 128-round windows: the lists
    equal the rule on dgpu_verify_rows' outputs, and the list written out by
    hand -- the rows the device leaves are 40, 41 (JSON with whitespace), 60
    (not JSON), 120 and 130 (a field above its stride)."""
    from drand_amd import _lib
    from drand_amd.ingest import window_rows
    bs, c, want = planted
    m = getattr(_lib, mode)
    pk = np.frombuffer(c.pk, dtype=np.uint8).copy()
    end = bs.len()  # visited rounds 1 .. Len - 1
    assert end == 199
    by_hand = [(r, v) for r, v in want if r not in (41, 60, 120, 130) and r < end]
    left_by_hand = [40, 41, 60, 120, 130]
    for size in (end - 1, 128):
        got_f, got_left = [], []
        for lo in range(1, end, size):
            rows = window_rows(bs, lo, min(end, lo + size))
            first, count = rows.lo, rows.hi - rows.lo
            rounds, ok, reason = verify_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, rows.buf, rows.off, rows.len, 96, 96, m, 7)
            w = rule(first, count, rows.keys, ok, rounds, reason)
            pos, val, left, totals, rs = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, rows.buf, rows.off, rows.len,
                                                    rows.keys, 96, 96, m, 7, first, count, reason=True)
            assert np.array_equal(pos, w[0]) and np.array_equal(val, w[1]) and np.array_equal(left, w[2])
            assert totals == [len(w[0]), len(w[2])] and np.array_equal(rs, reason)
            # staged: dgpu_verify_rows' bytes and 8 per key
            assert _lib.staging_stats(gpu_ctx)[2] == int(rows.len.sum()) + 20 * len(rows.off)
            got_f += [(first + int(p), int(v)) for p, v in zip(pos, val)]
            got_left += [int(rows.keys[int(r)]) for r in left]
            # caps below the totals
            tp, tv, tl, tt = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, rows.buf, rows.off, rows.len, rows.keys, 96,
                                        96, m, 7, first, count, fcap=len(w[0]) // 2, lcap=1)
            assert tt == totals and np.array_equal(tp, w[0][:len(w[0]) // 2]) and np.array_equal(tl, w[2][:1])
        assert got_f == by_hand and got_left == left_by_hand, size


def fixture_rows(name, total):
    """About `total` rows of a golden chain fixture under consecutive keys: its
    valid rounds and every corruption kind, repeated, with non-canonical and
    garbage rows mixed in and some keys skipped (missing rounds)."""
    g = load_golden(name)

    def b(x, none_if_empty=False):
        v = bytes.fromhex(x)
        return None if (none_if_empty and not v) else v
    chained = g["scheme"] == "pedersen-bls-chained"
    items = list(g["rounds"]) + list(g["corrupted"])
    rows, keys, k = [], [], 0
    while len(rows) < total:
        r = items[k % len(items)]
        row = marshal(b(r["prev"], not chained), r["round"], b(r["sig"]))
        if k % 41 == 7:
            row = json.dumps({"PreviousSig": r["prev"], "Round": r["round"], "Signature": r["sig"]}).encode()
        elif k % 53 == 11:
            row = os.urandom(1 + k % 300)
        elif k % 67 == 13:
            row = b""
        if k % 29 != 5:  # (a skipped key: a missing round)
            rows.append(row)
            keys.append(500 + k)
        k += 1
    return np.frombuffer(bytes.fromhex(g["pk"]), dtype=np.uint8).copy(), rows, np.array(keys, dtype=np.uint64), 500 + k


@pytest.mark.parametrize("name,scheme,strides,mode", [
    ("chain_chained_s1.json", "SCHEME_CHAINED", (96, 96), "MODE_PER_ROUND"),
    ("chain_chained_s1.json", "SCHEME_CHAINED", (96, 96), "MODE_RLC"),
    ("chain_unchained_s1.json", "SCHEME_UNCHAINED", (96, 48), "MODE_PER_ROUND"),
    ("chain_on_g1_s1.json", "SCHEME_UNCHAINED_G1", (48, 48), "MODE_RLC")])
def test_check_rows_golden_fixtures(name, scheme, strides, mode):
    """The golden fixtures with every corruption kind they carry (stored
    Rounds differ from the keys throughout): the rule on dgpu_verify_rows'
    outputs, on a context whose RLC calls take the RLC path."""
    from drand_amd import _lib
    pk, rows, keys, end = fixture_rows(name, 600)
    buf, off, ln = pack(rows, lead=b"\0" * 3)
    with contextlib.closing(open_ctx({"DGPU_RLC_MIN": "0"})) as ctx:
        code, m = getattr(_lib, scheme), getattr(_lib, mode)
        rounds, ok, reason = verify_rows(ctx, code, pk, buf, off, ln, *strides, m, 0x1234)
        first, count = 498, end + 3 - 498  # missing rounds in front of the first key and behind the last
        w = rule(first, count, keys, ok, rounds, reason)
        pos, val, left, totals, rs = check_rows(ctx, code, pk, buf, off, ln, keys, *strides, m, 0x1234, first, count,
                                                reason=True)
        assert np.array_equal(pos, w[0]) and np.array_equal(val, w[1]) and np.array_equal(left, w[2])
        assert np.array_equal(rs, reason) and (reason == 0).any() and len(set(reason.tolist())) >= 3
        assert len(left) > 10 and 20 < len(pos) < count and (val != first + pos).any()
        assert pos[:2].tolist() == [0, 1] and pos[-1] == count - 1


def test_check_rows_argument_errors_leave_the_context_working(gpu_ctx):
    from drand_amd import _lib
    g = load_golden("chain_chained_s1.json")
    pk = np.frombuffer(bytes.fromhex(g["pk"]), dtype=np.uint8).copy()
    rows = [marshal(bytes.fromhex(r["prev"]), r["round"], bytes.fromhex(r["sig"])) for r in g["rounds"][:6]]
    buf, off, ln = pack(rows)
    keys = np.arange(10, 16, dtype=np.uint64)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    out = np.zeros(16, dtype=np.uint64)
    cnt = np.zeros(2, dtype=np.uint64)

    def call(keys_, first, count, buf_=buf, lists=True, nf=True):
        P = _lib.ptr
        return lib.dgpu_check_rows(h, _lib.SCHEME_CHAINED, P(pk), pk.size, len(keys_), P(buf_), P(off), P(ln), P(keys_), 96,
                                   96, 0, 0, first, count, P(out) if lists else None, P(out[8:]) if lists else None, 8,
                                   P(cnt) if nf else None, P(out), 0, P(cnt[1:]), None)

    def works():
        pos, val, left, totals = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, buf, off, ln, keys, 96, 96, 0, 0, 9, 8)
        assert (pos.tolist(), val.tolist(), left.tolist()) == ([0, 7], [9, 16], [])
    works()
    bad = [call(np.array([10, 11, 11, 13, 14, 15], dtype=np.uint64), 9, 8),  # not strictly ascending
           call(np.array([10, 11, 13, 12, 14, 15], dtype=np.uint64), 9, 8),
           call(keys, 11, 8),                                               # a key below first
           call(keys, 9, 6),                                                # a key at first + count
           call(keys + np.uint64(2 ** 64 - 20), 2 ** 64 - 12, 20),          # first + count overflows
           call(keys, 9, 8, buf_=None), call(keys, 9, 8, lists=False), call(keys, 9, 8, nf=False)]
    assert bad == [_lib.DGPU_EINVAL] * len(bad)
    works()
    # n = 0: every position faulty; count = 0: two zero totals, NULL everywhere else
    empty = np.zeros(0, dtype=np.uint64)
    pos, val, left, totals = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, np.zeros(0, dtype=np.uint8), empty,
                                        np.zeros(0, dtype=np.uint32), empty, 96, 96, 0, 0, 5, 3)
    assert (pos.tolist(), val.tolist(), totals) == ([0, 1, 2], [5, 6, 7], [3, 0])
    cnt[:] = 9
    _lib.check(lib.dgpu_check_rows(h, _lib.SCHEME_CHAINED, _lib.ptr(pk), pk.size, 0, None, None, None, None, 96, 96, 0, 0,
                                   5, 0, None, None, 0, _lib.ptr(cnt), None, 0, _lib.ptr(cnt[1:]), None), lib)
    assert cnt.tolist() == [0, 0]
    works()


# ---------------------------------------------------------------- check_past_beacons(replay="device")
@pytest.mark.parametrize("mode", ["MODE_PER_ROUND", "MODE_RLC"])
def test_check_past_beacons_replay_device_equals_replay_host(planted, mode):
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.sync import check_past_beacons
    bs, c, want = planted
    v = Verifier(get_scheme_by_id_with_default("pedersen-bls-chained"), device=0)
    m = getattr(_lib, mode)
    length = bs.len()
    for up_to in (0, 1, 101, length - 1, length + 5):
        end = min(length, max(up_to, 1) + 1)
        expect = [val for r, val in want if r < end] or None
        calls = {}
        for key, kw in (("host", dict(decode="host")), ("device", dict(decode="device")),
                        ("replay", dict(decode="device", replay="device"))):
            calls[key] = []
            got = check_past_beacons(bs, v, c.pk, up_to, cb=lambda i, u, k=key: calls[k].append((i, u)), window=128,
                                     mode=m, **kw)
            assert got == expect, (key, up_to, got)
        assert calls["replay"] == calls["host"] == calls["device"] and len(calls["host"]) == end - 1
        for window in (128, None):  # without callbacks: a path of its own
            assert check_past_beacons(bs, v, c.pk, up_to, window=window, mode=m, decode="device",
                                      replay="device") == expect
