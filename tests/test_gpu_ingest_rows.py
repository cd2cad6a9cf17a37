"""Stored beacon rows decoded on the GPU (k_ingest_rows; dgpu_decode_rows_device,
dgpu_verify_rows, check_past_beacons(decode="device")).

The yardstick is the native host decoder (dgpu_ingest_decode, alone: without
ingest.decode's beacon_unmarshal pass): the device decoder's records equal its
records byte for byte, dgpu_verify_rows equals dgpu_verify_beacons on the
arrays it writes, and the check-chain loop over a bolt file returns the same
faulty rounds and makes the same callbacks whichever side decodes."""
import contextlib
import json
import os
import struct

import numpy as np
import pytest

from bolt_writer import write_bolt
from conftest import load_golden, open_ctx
from ingest_rows_corpus import corpus, marshal, pack

pytestmark = pytest.mark.gpu
SLOT = 16 << 20  # the pinned ring's slot (include/drand_gpu.h, dgpu_verify_rows)


def native_decode(buf, off, ln, sig_stride, prev_stride):
    """dgpu_ingest_decode alone: (rounds, sigs, sig_len, prev, prev_len, ok)."""
    from drand_amd import ingest
    L = ingest.load()
    n = len(off)
    rounds = np.zeros(n, dtype=np.uint64)
    sigs = np.zeros((n, sig_stride), dtype=np.uint8)
    sig_len = np.zeros(n, dtype=np.uint32)
    prev = np.zeros((n, prev_stride), dtype=np.uint8)
    prev_len = np.zeros(n, dtype=np.uint32)
    ok = np.zeros(n, dtype=np.uint8)
    if n:
        L.dgpu_ingest_decode(n, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, rounds.ctypes.data, sigs.ctypes.data,
                             sig_stride, sig_len.ctypes.data, prev.ctypes.data, prev_stride, prev_len.ctypes.data,
                             ok.ctypes.data)
    return rounds, sigs, sig_len, prev, prev_len, ok


@pytest.fixture(scope="module")
def stored_rows(tmp_path_factory):
    """The rows of two bolt files (4 KiB and 1 KiB pages, both with branch
    levels), read back through the store's scan, then the corpus at 96 / 96."""
    from drand_amd.boltstore import BoltStore
    rng = np.random.default_rng(5)
    tmp = tmp_path_factory.mktemp("rows")
    rows = []
    for page_size, count in ((4096, 700), (1024, 300)):
        kv = {struct.pack(">Q", r): marshal(rng.bytes(96 if r > 1 else 32), r, rng.bytes(96)) for r in range(1, count + 1)}
        p = tmp / f"db{page_size}"
        write_bolt(p, kv, page_size=page_size)
        bs = BoltStore(p)
        rr, off, ln, buf = bs.scan_offsets(1, count + 1)
        assert rr.tolist() == list(range(1, count + 1))
        got = [bytes(buf[int(o):int(o) + int(l)]) for o, l in zip(off, ln)]
        assert got == [kv[struct.pack(">Q", r)] for r in range(1, count + 1)]
        rows += got
        bs.close()
    return rows + [r for _, r in corpus(96, 96)]


def device_decode(gpu_ctx, buf, off, ln, sig_stride, prev_stride, shift=0):
    """dgpu_decode_rows_device on a device copy of buf that starts `shift`
    bytes into its allocation; the record arrays carry 64 guard bytes."""
    import torch
    from drand_amd import calls
    n = len(off)
    G = 64
    whole = torch.zeros(buf.size + shift, dtype=torch.uint8, device="cuda")
    d_rows = whole[shift:]
    d_rows.copy_(torch.from_numpy(buf))
    d_off, d_len = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ln.view(np.int32)).cuda()
    out = {k: torch.full((size + G,), 0xA5, dtype=torch.uint8, device="cuda")
           for k, size in (("rounds", 8 * n), ("sigs", n * sig_stride), ("sig_len", 4 * n), ("prev", n * prev_stride),
                           ("prev_len", 4 * n), ("ok", n))}
    calls.decode_rows_device(gpu_ctx, d_rows, d_off, d_len, out["rounds"], out["sigs"], out["sig_len"], out["prev"],
                             out["prev_len"], out["ok"], sig_stride=sig_stride, prev_stride=prev_stride)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert (v[-G:] == 0xA5).all(), f"{k}: written past the array"
    return (host["rounds"][:-G].view(np.uint64), host["sigs"][:-G].reshape(n, sig_stride),
            host["sig_len"][:-G].view(np.uint32), host["prev"][:-G].reshape(n, prev_stride),
            host["prev_len"][:-G].view(np.uint32), host["ok"][:-G])


def assert_records_equal(got, want):
    for name, g, w in zip(("rounds", "sigs", "sig_len", "prev", "prev_len", "ok"), got, want):
        assert np.array_equal(g, w), (name, np.nonzero(np.atleast_1d((g != w).reshape(len(w), -1).any(axis=1)))[0][:10])


@pytest.mark.parametrize("oob", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_device_decoder_equals_native_decoder(stored_rows, gpu_ctx, n, oob):
    """Record-by-record byte equality and equal ok.  The packed buffer is
    exactly the rows' bytes behind three lead bytes (no row starts on a
    multiple of 16 by construction of the lengths; the last row ends on the
    buffer's last byte), copied to a device allocation at an odd address.
    oob: one more row whose range points past the buffer -- it is not read
    and decodes to a zeroed record; its wave takes the direct path."""
    step = max(1, len(stored_rows) // n)
    rows = stored_rows[::step][:n] if n > 65 else (stored_rows[:n // 2] + stored_rows[-(n - n // 2):])
    buf, off, ln = pack(rows, lead=b"\xff\xfe\xfd")
    assert off[-1] + ln[-1] == buf.size and len(rows) == n
    assert n < 64 or (off % 16 != 0).mean() > 0.8
    want = list(native_decode(buf, off, ln, 96, 96))
    if oob:
        at = n // 2
        off = np.insert(off, at, buf.size - 10)
        ln = np.insert(ln, at, 100)
        for k, w in enumerate(want):
            want[k] = np.insert(w, at, 0, axis=0)
    got = device_decode(gpu_ctx, buf, off, ln, 96, 96, shift=1)
    assert_records_equal(got, want)
    assert oob or n == 1 or got[5].sum() > 0


@pytest.mark.parametrize("strides", [(48, 96), (97, 98), (96, 0)])
def test_device_decoder_strides_and_row_order(stored_rows, gpu_ctx, strides):
    """Other strides (48: the G1 signatures; 97 / 98: no whole words, the
    byte stores; prev_stride 0), the corpus built at those strides, and rows
    listed in no order with repeats (the direct path) beside ordered runs."""
    ss, ps = strides
    rows = stored_rows[:200] + [r for _, r in corpus(ss, max(ps, 1))][:600]
    buf, off, ln = pack(rows)
    order = np.arange(len(rows))
    rng = np.random.default_rng(9)
    order[64:192] = rng.integers(0, len(rows), 128)  # two waves of unordered, repeated rows
    off, ln = np.ascontiguousarray(off[order]), np.ascontiguousarray(ln[order])
    want = native_decode(buf, off, ln, ss, ps)
    got = device_decode(gpu_ctx, buf, off, ln, ss, ps)
    assert_records_equal(got, want)
    assert 0 < got[5].sum() < len(rows)


def test_device_decoder_rows_beyond_the_lds_budget(gpu_ctx):
    """130 ordered rows of about 850 bytes at strides 200 / 200: 64 of them are 52 KB,
    beyond the 30 KB a wave stages, so every wave reads global memory directly."""
    rng = np.random.default_rng(11)
    rows = [marshal(rng.bytes(200), 10 ** 6 + i, rng.bytes(200 if i % 7 else 96)) for i in range(130)]
    buf, off, ln = pack(rows, lead=b"\x01")
    assert int(ln[:64].sum()) > 30720
    want = native_decode(buf, off, ln, 200, 200)
    assert want[5].all()
    assert_records_equal(device_decode(gpu_ctx, buf, off, ln, 200, 200, shift=3), want)


def test_device_decoder_empty_call(gpu_ctx):
    from drand_amd import _lib
    _lib.check(gpu_ctx.lib.dgpu_decode_rows_device(gpu_ctx.handle, 0, None, 0, None, None, None, None, 96, None, None, 96,
                                                   None, None, None), gpu_ctx.lib)


# ---------------------------------------------------------------- dgpu_verify_rows
def verify_rows(ctx, code, pk, buf, off, ln, sig_stride, prev_stride, mode, seed):
    """(rounds, row_ok, reasons) of dgpu_verify_rows, every output sentinel-filled before the call."""
    from drand_amd import calls
    reason, ok, rounds = calls.verify_rows(ctx, code, pk, buf, off, ln, sig_stride, prev_stride, mode, seed, fill=0xEE)
    return rounds, ok, reason


def verify_records(ctx, code, pk, rec, mode, seed):
    """dgpu_verify_beacons on native_decode's arrays."""
    from drand_amd import calls
    return calls.verify_beacons(ctx, code, pk, *rec[:5], mode, seed, fill=0xEE)


def fixture_rows(name, total):
    """About `total` rows from a golden chain fixture: its valid rounds and
    every corruption kind, repeated, with non-canonical and garbage rows mixed
    in.  Returns (pk, rows, expected reason per row or None where the row is
    not canonical)."""
    g = load_golden(name)

    def b(x, none_if_empty=False):
        v = bytes.fromhex(x)
        return None if (none_if_empty and not v) else v
    chained = g["scheme"] == "pedersen-bls-chained"
    items = [(r, 0) for r in g["rounds"]] + [(c, c["reason"]) for c in g["corrupted"]]
    rows, expect = [], []
    k = 0
    while len(rows) < total:
        r, reason = items[k % len(items)]
        row = marshal(b(r["prev"], not chained), r["round"], b(r["sig"]))
        if k % 41 == 7:  # a valid beacon stored as JSON with whitespace: not canonical
            row = json.dumps({"PreviousSig": r["prev"], "Round": r["round"], "Signature": r["sig"]}).encode()
            reason = None
        elif k % 53 == 11:
            row, reason = os.urandom(1 + k % 300), None
        elif k % 67 == 13:
            row, reason = b"", None
        elif k % 71 == 17:  # longer than any canonical row at the strides: not staged
            row, reason = row[:-2] + b"00" * 400 + b'"}', None
        rows.append(row)
        expect.append(reason)
        k += 1
    return np.frombuffer(bytes.fromhex(g["pk"]), dtype=np.uint8).copy(), rows, expect


def check_rows_against_records(ctx, code, pk, rows, expect, sig_stride, prev_stride, mode, seed=0x1234):
    from drand_amd import _lib
    buf, off, ln = pack(rows, lead=b"\0" * 7)
    rec = native_decode(buf, off, ln, sig_stride, prev_stride)
    w_reason = verify_records(ctx, code, pk, rec, mode, seed)
    rounds, ok, reason = verify_rows(ctx, code, pk, buf, off, ln, sig_stride, prev_stride, mode, seed)
    assert np.array_equal(ok, rec[5]) and np.array_equal(rounds, rec[0])
    assert np.array_equal(reason, w_reason)  # (the bitmaps too: each call checks its own against its reasons)
    # and the verdicts are the fixture's: a row that is not canonical is a decode failure
    want = [_lib.REASON_DECODE if e is None else e for e in expect]
    canon = [e is not None for e in expect]
    over = [e is not None and not o for e, o in zip(expect, ok)]  # canonical JSON, a field above its stride
    assert ok.tolist() == [int(c and not v) for c, v in zip(canon, over)]
    assert [r for r, v in zip(reason.tolist(), over) if not v] == [w for w, v in zip(want, over) if not v]
    assert all(reason[i] == _lib.REASON_DECODE for i, v in enumerate(over) if v)
    return reason


@pytest.mark.parametrize("mode", ["MODE_PER_ROUND", "MODE_RLC"])
def test_verify_rows_equals_verify_beacons_chained(mode):
    """The golden chained fixture with every corruption kind, non-canonical
    and garbage rows mixed in, n = 1,000; RLC mode on the RLC path itself
    (DGPU_RLC_MIN lowered on a context of its own)."""
    from drand_amd import _lib
    pk, rows, expect = fixture_rows("chain_chained_s1.json", 1000)
    with contextlib.closing(open_ctx({"DGPU_RLC_MIN": "0"})) as ctx:
        reason = check_rows_against_records(ctx, _lib.SCHEME_CHAINED, pk, rows, expect, 96, 96, getattr(_lib, mode))
        assert (reason == 0).sum() > 500 and len(set(reason.tolist())) == 5


@pytest.mark.parametrize("name,scheme,strides", [("chain_unchained_s1.json", "SCHEME_UNCHAINED", (96, 48)),
                                                 ("chain_on_g1_s1.json", "SCHEME_UNCHAINED_G1", (48, 48))])
def test_verify_rows_unchained_and_g1_at_stride_48(gpu_ctx, name, scheme, strides):
    """The unchained fixture with its (unused) previous signatures at stride
    48 and the on-G1 fixture with both strides 48: its G2-sized signature is
    then above the stride -- not canonical, a decode failure either way."""
    from drand_amd import _lib
    pk, rows, expect = fixture_rows(name, 300)
    check_rows_against_records(gpu_ctx, getattr(_lib, scheme), pk, rows, expect, *strides, _lib.MODE_PER_ROUND)


def test_verify_rows_empty_and_bad_arguments(gpu_ctx):
    from drand_amd import _lib
    pk = np.frombuffer(bytes.fromhex(load_golden("chain_chained_s1.json")["pk"]), dtype=np.uint8).copy()
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    _lib.check(lib.dgpu_verify_rows(h, _lib.SCHEME_CHAINED, _lib.ptr(pk), pk.size, 0, None, None, None, 96, 96, 0, 0, None,
                                    None, None, None), lib)
    buf, off, ln = pack([b"{}"])
    out = np.zeros(8, dtype=np.uint8)
    for ss, args in ((48, (_lib.ptr(buf), _lib.ptr(off), _lib.ptr(ln))), (96, (None, _lib.ptr(off), _lib.ptr(ln)))):
        rc = lib.dgpu_verify_rows(h, _lib.SCHEME_CHAINED, _lib.ptr(pk), pk.size, 1, *args, ss, 96, 0, 0, None,
                                  _lib.ptr(out), _lib.ptr(out), None)
        assert rc == _lib.DGPU_EINVAL


# ---------------------------------------------------------------- ring pieces
def piece_cuts(ln, max_len):
    """dgpu_verify_rows' pieces: the longest runs of whole rows whose packed
    bytes (over-long rows take none), rounded up to 8, plus 12 bytes per row
    fit a ring slot."""
    staged = np.where(ln <= max_len, ln, 0).astype(np.int64)
    cuts, a, n = [0], 0, len(ln)
    pos = np.concatenate([[0], np.cumsum(staged)])
    while a < n:
        e = a + 1
        while e < n and ((pos[e + 1] - pos[a] + 7) // 8) * 8 + 12 * (e + 1 - a) <= SLOT:
            e += 1
        cuts.append(e)
        a = e
    return cuts, int(staged.sum())


def test_verify_rows_across_ring_pieces(gpu_ctx):
    """80,001 chained rows, about 35 MB: three ring pieces.  Corruptions
    planted in the first and the last row of every piece (and an over-long
    row, which is not staged); the verdicts equal the explicit-record call's
    on the same chain, and dgpu_staging_stats reports the documented bytes."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    n = 80001
    c = make_chain(31, n, _lib.SCHEME_CHAINED, seg_len=64)
    pk = np.frombuffer(c.pk, dtype=np.uint8).copy()
    sig_hex, prev_hex = c.sigs.tobytes().hex(), c.prev.tobytes().hex()
    rows = [('{"PreviousSig":"%s","Round":%d,"Signature":"%s"}' %
             (prev_hex[192 * i:192 * i + 2 * int(c.prev_len[i])], int(c.rounds[i]), sig_hex[192 * i:192 * i + 192])).encode()
            for i in range(n)]
    ln0 = np.array([len(r) for r in rows], dtype=np.uint32)
    cuts, _ = piece_cuts(ln0, 64 + 2 * (96 + 96))
    assert len(cuts) - 1 >= 3, cuts
    planted = sorted({i for a, b in zip(cuts, cuts[1:]) for i in (a, b - 1)})
    for i in planted:  # another hex digit in the signature's x coordinate
        r = bytearray(rows[i])
        at = len(r) - 2 - 100
        r[at] = ord("0") if r[at] != ord("0") else ord("1")
        rows[i] = bytes(r)
        c.sigs[i] = np.frombuffer(bytes.fromhex(rows[i][-194:-2].decode()), dtype=np.uint8)
    long_row = cuts[1] + 5
    rows[long_row] = rows[long_row][:-2] + b"0" * 2000 + b'"}'
    c.sigs[long_row], c.sig_len[long_row], c.prev[long_row], c.prev_len[long_row], c.rounds[long_row] = 0, 0, 0, 0, 0
    buf, off, ln = pack(rows, lead=b"\0" * 5)
    rounds, ok, reason = verify_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, buf, off, ln, 96, 96, _lib.MODE_PER_ROUND, 0)
    ms, host_ms, nbytes = _lib.staging_stats(gpu_ctx)
    _, staged = piece_cuts(ln, 64 + 2 * (96 + 96))
    assert nbytes == staged + 12 * n and staged == int(ln.sum()) - int(ln[long_row]) and ms > 0 and host_ms > 0
    w_reason = verify_records(gpu_ctx, _lib.SCHEME_CHAINED, pk, c.records(), _lib.MODE_PER_ROUND, 0)
    assert np.array_equal(reason, w_reason)
    assert np.array_equal(rounds, c.rounds)
    expect_ok = np.ones(n, dtype=np.uint8)
    expect_ok[long_row] = 0
    assert np.array_equal(ok, expect_ok)
    assert np.nonzero(reason)[0].tolist() == sorted(planted + [long_row])


# ---------------------------------------------------------------- check_past_beacons
@pytest.mark.parametrize("mode", ["MODE_PER_ROUND", "MODE_RLC"])
def test_check_past_beacons_device_decode_equals_host_decode(tmp_path, gpu_ctx, mode):
    """A bolt file with missing rows, a valid and a corrupted beacon stored as
    JSON with whitespace, an undecodable row, corrupted signatures, a
    signature and a previous signature above the stride, and a row whose
    Round differs from its key: identical faulty lists and callback
    sequences, with and without a callback, over several windows."""
    from drand_amd import _lib
    from drand_amd.boltstore import BoltStore
    from drand_amd.chain import Beacon, Verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.sync import MemoryStore, beacon_marshal, check_past_beacons
    from drand_amd.synth import make_chain
    n, window = 200, 128
    c = make_chain(77, n, _lib.SCHEME_CHAINED, seg_len=8)  # (a stored row carries its own previous signature)
    st = MemoryStore()
    st.put(Beacon(b"", 0, c.genesis))

    def beacon(i, round_=None, sig=None, prev=None):  # chain item i = round i + 1
        return Beacon(bytes(c.prev[i, :c.prev_len[i]]) if prev is None else prev, int(c.rounds[i]) if round_ is None else round_,
                      bytes(c.sigs[i, :c.sig_len[i]]) if sig is None else sig)

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
        b"ROUND", b"Round").replace(b"SIGNATURE", b"Signature"))  # upper-case hex: canonical, valid
    p = tmp_path / "drand.db"
    write_bolt(p, dict(st._kv))
    bs = BoltStore(p)
    v = Verifier(get_scheme_by_id_with_default("pedersen-bls-chained"), device=0)
    m = getattr(_lib, mode)
    # (visited round, its faulty value); the loop visits rounds 1 .. min(Len - 1, up_to)
    want = [(17, 17), (41, 41), (60, 60), (80, 80), (81, 81), (100, 107), (120, 120), (130, 130), (150, 150)]
    assert bs.len() == n + 1 - 2
    for up_to in (n,):
        end = min(bs.len(), up_to + 1)
        expect = [val for r, val in want if r < end]
        calls = {}
        for decode in ("host", "device"):
            calls[decode] = []
            got = check_past_beacons(bs, v, c.pk, up_to, cb=lambda i, u, d=decode: calls[d].append((i, u)), window=window,
                                     mode=m, decode=decode)
            assert got == expect, (decode, got)
            if up_to == n:  # the replay without callbacks is a path of its own
                assert check_past_beacons(bs, v, c.pk, up_to, window=window, mode=m, decode=decode) == expect
        assert calls["host"] == calls["device"] and len(calls["host"]) == end - 1
    with pytest.raises(ValueError):
        check_past_beacons(st, v, c.pk, n, decode="device")
    bs.close()
