"""dgpu_check_rows_multi and MultiVerifier.verify_rows over D = 2 and 3
contexts on one GPU (DGPU_MULTI_ALLOW_SAME_DEVICE=1: every multi-device branch
runs; the RCCL all-gathers are in-library copies).  The yardstick is
dgpu_check_rows on one context: the lists are equal element for element, in
both modes.  The store's faults sit on the shard boundaries: missing rounds at
lo_k - 1, lo_k and lo_k + 1, a faulty row as the last item of shard 0 and
another as the first item of shard 1, the last row missing.  RCCL with two or
more real ranks is unmeasured."""
import numpy as np
import pytest

from ingest_rows_corpus import marshal
from test_gpu_check_rows import check_rows, pack, rule, verify_rows

pytestmark = pytest.mark.gpu
N_KEYS = 150  # rounds 1 .. 150 before the removals


@pytest.fixture(scope="module")
def chain150():
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    return make_chain(91, N_KEYS, _lib.SCHEME_CHAINED, seg_len=8)


def store_rows(c, missing, faulty, left=()):
    """(rows, keys): the chain's rounds without `missing`; `faulty` rounds
    carry a corrupted signature under another Round, `left` rounds a row that
    is not canonical."""
    rows, keys = [], []
    for i in range(N_KEYS):
        r = i + 1
        if r in missing:
            continue
        sig = bytearray(c.sigs[i, :c.sig_len[i]].tobytes())
        rnd = r
        if r in faulty:
            sig[40] ^= 4
            rnd = r + 5000
        row = marshal(bytes(c.prev[i, :c.prev_len[i]]), rnd, bytes(sig))
        if r in left:
            row = row.replace(b'"Round":', b'"Round": ')
        rows.append(row)
        keys.append(r)
    return rows, np.array(keys, dtype=np.uint64)


def boundary_store(c, ndev):
    """Faults placed by the shard cuts of the rows that remain (the cuts are
    multiples of 8 rows and do not depend on which rounds are missing once
    their number is fixed)."""
    from drand_amd import _lib
    n_missing = 3 * (ndev - 1) + 1
    n = N_KEYS - n_missing
    assert n % 8 != 0
    cuts = [_lib.shard_range(n, ndev, k) for k in range(ndev)]
    # build the key list so that the rounds around each later shard's first key are missing:
    # rows before the cut keep their rounds; at cut k the rounds r - 1, r, r + 1 are dropped
    missing, keys, r = set(), [], 1
    for k, (lo, hi) in enumerate(cuts):
        if k:
            missing |= {r, r + 1, r + 2}  # lo_k - 1, lo_k, lo_k + 1 in round numbers, were the rows all there
            r += 3
        keys += list(range(r, r + hi - lo))
        r += hi - lo
    missing.add(N_KEYS)  # the last row
    assert r == N_KEYS and len(keys) == n and len(missing) == n_missing
    faulty = {keys[cuts[0][1] - 1], keys[cuts[1][0]], keys[5]}  # last of shard 0, first of shard 1
    left = {keys[cuts[0][1] - 2], keys[cuts[1][0] + 1], keys[-1]}
    rows, got = store_rows(c, missing, faulty, left)
    assert got.tolist() == keys
    return rows, got, cuts, faulty


@pytest.mark.parametrize("ndev", [2, 3])
def test_check_rows_multi_equals_single(ndev, chain150, gpu_ctx, monkeypatch):
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.ingest import Rows
    from drand_amd.multi import MultiVerifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    c = chain150
    pk = np.frombuffer(c.pk, dtype=np.uint8).copy()
    rows, keys, cuts, faulty = boundary_store(c, ndev)
    buf, off, ln = pack(rows, lead=b"\0" * 5)
    n, first, count = len(rows), 1, N_KEYS
    sch = get_scheme_by_id_with_default("pedersen-bls-chained")
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(sch, [0] * ndev)
    v = Verifier(sch)
    try:
        multi = lambda *a: mv.mctx.lib.dgpu_check_rows_multi(mv.mctx.handle, *a)  # noqa: E731
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            single = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, buf, off, ln, keys, 96, 96, mode, 77, first, count,
                                reason=True)
            got = check_rows(mv.mctx, _lib.SCHEME_CHAINED, pk, buf, off, ln, keys, 96, 96, mode, 77, first, count,
                             reason=True, call=multi)
            for name, g, w in zip(("pos", "val", "left", "totals", "reason"), got, single):
                assert np.array_equal(g, w), (mode, name, g, w)
            # ... and they are the planted ones: every missing round, the three corrupted rows under their stored Round
            pos, val, left = got[:3]
            gone = sorted(set(range(1, N_KEYS + 1)) - set(keys.tolist()))
            want = sorted([(r - 1, r) for r in gone] + [(r - 1, r + 5000) for r in faulty])
            assert list(zip(pos.tolist(), val.tolist())) == want and len(left) == 3
            assert {cuts[0][1] - 1, cuts[1][0]} <= {int(np.nonzero(keys == r)[0][0]) for r in faulty}
            # caps below the totals cut the concatenation, not each device's list
            cut = check_rows(mv.mctx, _lib.SCHEME_CHAINED, pk, buf, off, ln, keys, 96, 96, mode, 77, first, count,
                             fcap=len(pos) - 2, lcap=2, call=multi)
            assert cut[3] == got[3] and np.array_equal(cut[0], pos[:-2]) and np.array_equal(cut[1], val[:-2])
            assert np.array_equal(cut[2], left[:2])
            # each shard's rows and keys went through its context's ring
            for k, (lo, hi) in enumerate(cuts):
                ctx_k = mv._shard_verifiers()[k].ctx
                assert _lib.staging_stats(ctx_k)[2] == int(ln[lo:hi].sum()) + 20 * (hi - lo), (mode, k)
            # MultiVerifier.verify_rows and check_rows
            reasons, ok, rounds = mv.verify_rows(c.pk, buf, off, ln, mode, 77)
            w_reasons, w_ok, w_rounds = v.verify_rows(c.pk, buf, off, ln, mode, 77)
            assert np.array_equal(reasons, w_reasons) and np.array_equal(ok, w_ok) and np.array_equal(rounds, w_rounds)
            assert np.array_equal(reasons, got[4])
            r3 = mv.check_rows(c.pk, Rows(first, first + count, keys, off, ln, buf), first, count, mode, 77)
            assert all(np.array_equal(a, b) for a, b in zip(r3, got[:3]))
        # an empty last shard: 8 rows over 3 devices (shards of 8, 0, 0), and a window that ends past the rows
        few = slice(0, 8)
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            if ndev == 3:
                assert _lib.shard_range(8, ndev, 2) == (8, 8)
            a = check_rows(gpu_ctx, _lib.SCHEME_CHAINED, pk, buf, off[few], ln[few], keys[few], 96, 96, mode, 5, 1, 12)
            b = check_rows(mv.mctx, _lib.SCHEME_CHAINED, pk, buf, off[few], ln[few], keys[few], 96, 96, mode, 5, 1, 12,
                           call=multi)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].tolist()[-4:] == [8, 9, 10, 11]
        # n = 0: shard 0 owns every position
        e64, e32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
        z = check_rows(mv.mctx, _lib.SCHEME_CHAINED, pk, np.zeros(0, dtype=np.uint8), e64, e32, e64, 96, 96, 0, 0, 7, 3,
                       call=multi)
        assert (z[0].tolist(), z[1].tolist(), z[3]) == ([0, 1, 2], [7, 8, 9], [3, 0])
    finally:
        mv.close()
