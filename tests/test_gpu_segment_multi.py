"""dgpu_verify_segment_multi (MultiVerifier.verify_segment): a linked segment
over D = 2, 3 and 8 contexts on one GPU (DGPU_MULTI_ALLOW_SAME_DEVICE=1: the
all-gathers become in-library device copies, every other line is the
production D >= 2 path).  Shard 0 verifies from the caller's seed, shard k > 0
from its halo -- record lo_k - 1 of the caller's arrays, staged by the library
ahead of the shard.  Reasons and randomness must equal the single-context
Verifier.verify_segment bit for bit, in both modes, and the construction.

The chain is tests/test_gpu_multi.py's: 5003 rounds in 64-round generator
segments.  In the linked view a generator-segment start (i % 64 == 0, i > 0)
fails by construction (it was signed over a 32-byte seed, not over the
signature before it), so does every round whose signature or length was
corrupted, and the round after it, which hashes the altered record.  A
corruption of the explicit PreviousSig column has no array in the linked form:
those rounds stay valid here.  No shard boundary is a multiple of 64 (asserted),
so the first item of every later shard verifies only through a correct halo.
Marked gpu."""
import numpy as np
import pytest

from conftest import load_golden
from segment_helpers import check_randomness as _check_randomness

pytestmark = pytest.mark.gpu

N, SEG = 5003, 64
SHARD = {2: 2504, 3: 1672, 8: 632}


def _sch(name="pedersen-bls-chained"):
    from drand_amd.scheme import get_scheme_by_id_with_default
    return get_scheme_by_id_with_default(name)


def _linked_invalid(n, corrupted):
    """Expected-invalid set of a chained chain in the linked view."""
    return set(range(SEG, n, SEG)) | set(corrupted) | {i + 1 for i in corrupted if i + 1 < n}


@pytest.fixture(scope="module")
def chain5003():
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.synth import CORRUPT_PREV, CORRUPT_Y_SIGN, corrupt, make_chain
    c = make_chain(61, N, _lib.SCHEME_CHAINED, seg_len=SEG)
    clean_sigs, clean_len = c.sigs.copy(), c.sig_len.copy()
    bad = corrupt(c, 61, rate=2e-3)
    c.sigs[5, 0] ^= 0x20  # (as tests/test_gpu_multi.py: a bad round in the first shard at every D)
    bad[5] = CORRUPT_Y_SIGN
    corrupted = {i for i, kind in bad.items() if kind != CORRUPT_PREV}
    assert len(corrupted) < len(bad)  # (the PreviousSig kind is in the catalog, and leaves the linked view alone)
    expect = np.zeros(N, dtype=bool)
    expect[sorted(_linked_invalid(N, corrupted))] = True
    first, link = int(c.rounds[0]), bytes(c.prev[0, :c.prev_len[0]])
    v = Verifier(_sch())
    single = {}
    for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
        reasons, rand = v.verify_segment(first, c.sigs, link, c.pk, mode, 777, sig_len=c.sig_len)
        assert np.array_equal(reasons != 0, expect), mode  # every round has an expected verdict, by construction
        _check_randomness(rand, c.sigs, c.sig_len, reasons)
        single[mode] = (reasons, rand)
    assert np.array_equal(single[_lib.MODE_PER_ROUND][0], single[_lib.MODE_RLC][0])
    return c, expect, first, link, single, (clean_sigs, clean_len)


def _stats(mv, k):
    """dgpu_staging_stats of the handle's k-th context."""
    from drand_amd import _lib
    return _lib.staging_stats(mv._shard_verifiers()[k].ctx)


@pytest.mark.parametrize("ndev", [2, 3, 8])
def test_segment_multi_same_device_equals_single(ndev, chain5003, monkeypatch):
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.multi import MultiVerifier
    c, expect, first, link, single, (clean_sigs, clean_len) = chain5003
    stride = c.sigs.shape[1]
    lo_hi = [_lib.shard_range(N, ndev, k) for k in range(ndev)]
    assert lo_hi[0] == (0, SHARD[ndev])
    # no later shard starts on a generator-segment start: its first item needs the right halo
    assert all(lo % SEG != 0 and lo < N for lo, _ in lo_hi[1:])
    assert all(not expect[lo] for lo, _ in lo_hi[1:])  # ... and is expected to verify
    assert 0 < lo_hi[-1][1] - lo_hi[-1][0] < SHARD[ndev]  # a short last shard
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(_sch(), [0] * ndev)
    v = Verifier(_sch())
    try:
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            reasons, rand = mv.verify_segment(first, c.sigs, link, c.pk, mode, 12345, sig_len=c.sig_len)
            assert np.array_equal(reasons != 0, expect), mode
            assert np.array_equal(reasons, single[mode][0]), (mode, np.nonzero(reasons != single[mode][0])[0][:10])
            assert np.array_equal(rand, single[mode][1]), mode
            # each shard's signatures went through its context's ring once (the halo is staged beside them)
            for k, (lo, hi) in enumerate(lo_hi):
                assert _stats(mv, k)[2] == (hi - lo) * (stride + 4), (mode, k)
            r2, none = mv.verify_segment(first, c.sigs, link, c.pk, mode, 12345, randomness=False, sig_len=c.sig_len)
            assert none is None and np.array_equal(r2, reasons)
            # clean run: 56 consecutive rounds from inside one generator segment, seeded by
            # the signature before them; RLC passes on the summed node root alone.
            # D = 8: seven shards of 8 rounds, the last one empty
            a, b = SEG + 1, SEG + 57
            if ndev == 8:
                assert _lib.shard_range(b - a, ndev, ndev - 1) == (b - a, b - a)
            seed = bytes(clean_sigs[a - 1])
            reasons, rand = mv.verify_segment(first + a, clean_sigs[a:b], seed, c.pk, mode, 99, sig_len=clean_len[a:b])
            assert reasons.tolist() == [0] * (b - a)
            _check_randomness(rand, clean_sigs[a:b], clean_len[a:b], reasons)
            wrong = bytes([seed[0] ^ 1]) + seed[1:]
            reasons, _ = mv.verify_segment(first + a, clean_sigs[a:b], wrong, c.pk, mode, 99, sig_len=clean_len[a:b])
            assert reasons.tolist() == [_lib.REASON_PAIRING] + [0] * (b - a - 1)
            # a batch smaller than one shard
            reasons, rand = mv.verify_segment(first + a, clean_sigs[a:a + 5], seed, c.pk, mode, 99,
                                              sig_len=clean_len[a:a + 5])
            assert reasons.tolist() == [0] * 5
            want, want_rand = v.verify_segment(first + a, clean_sigs[a:a + 5], seed, c.pk, mode, 99,
                                               sig_len=clean_len[a:a + 5])
            assert reasons.tolist() == want.tolist() and np.array_equal(rand, want_rand)
    finally:
        mv.close()


def test_over_long_halo_record_is_a_decode_failure_of_two_rounds(chain5003, monkeypatch):
    """Record lo_1 - 1 has sig_len = stride + 4: rounds lo_1 - 1 (its own
    length) and lo_1 (its halo's length) fail with DGPU_REASON_DECODE; the
    call itself succeeds."""
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.multi import MultiVerifier
    c, _, first, link, _, (clean_sigs, clean_len) = chain5003
    lo1 = _lib.shard_range(N, 2, 1)[0]
    lens = clean_len.copy()
    lens[lo1 - 1] = clean_sigs.shape[1] + 4
    invalid = _linked_invalid(N, {lo1 - 1})
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(_sch(), [0, 0])
    try:
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            reasons, rand = mv.verify_segment(first, clean_sigs, link, c.pk, mode, 4242, sig_len=lens)
            assert set(np.nonzero(reasons)[0].tolist()) == invalid
            assert reasons[lo1 - 1] == reasons[lo1] == _lib.REASON_DECODE
            want, want_rand = Verifier(_sch()).verify_segment(first, clean_sigs, link, c.pk, mode, 4242, sig_len=lens)
            assert np.array_equal(reasons, want) and np.array_equal(rand, want_rand)
    finally:
        mv.close()


@pytest.mark.parametrize("name,code_name", [("pedersen-bls-unchained", "SCHEME_UNCHAINED"),
                                            ("bls-unchained-on-g1", "SCHEME_UNCHAINED_G1")])
def test_segment_multi_unchained_and_on_g1(name, code_name, monkeypatch):
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.multi import MultiVerifier
    from drand_amd.synth import corrupt, make_chain
    c = make_chain(62, 997, getattr(_lib, code_name), seg_len=SEG)
    bad = corrupt(c, 62, rate=5e-3)
    expect = np.zeros(len(c), dtype=bool)
    expect[sorted(bad)] = True  # previous signatures are ignored: only the corrupted rounds fail
    first = int(c.rounds[0])
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(_sch(name), [0, 0])
    v = Verifier(_sch(name))
    try:
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            reasons, rand = mv.verify_segment(first, c.sigs, b"", c.pk, mode, 31, sig_len=c.sig_len)
            assert np.array_equal(reasons != 0, expect), (name, mode)
            want, want_rand = v.verify_segment(first, c.sigs, b"", c.pk, mode, 31, sig_len=c.sig_len)
            assert np.array_equal(reasons, want) and np.array_equal(rand, want_rand), (name, mode)
            _check_randomness(rand, c.sigs, c.sig_len, reasons)
    finally:
        mv.close()


def test_segment_walk_takes_a_multi_verifier(monkeypatch):
    """sync.trusted_previous_signature_segments with a MultiVerifier returns
    what it returns with a Verifier (golden chained chain)."""
    from drand_amd.chain import VerifyError, new_verifier
    from drand_amd.multi import MultiVerifier
    from drand_amd.sync import trusted_previous_signature_segments
    g = load_golden("chain_chained_s1.json")
    pk = bytes.fromhex(g["pk"])
    sig = {r["round"]: bytes.fromhex(r["sig"]) for r in g["rounds"]}
    seed = bytes.fromhex(g["genesis"])
    v = new_verifier(_sch(g["scheme"]))
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(_sch(g["scheme"]), [0, 0, 0])
    try:
        for window in (7, 1 << 14):
            fetch = lambda lo, hi, s=sig: [s[r] for r in range(lo, hi + 1)]  # noqa: E731
            one = trusted_previous_signature_segments(v, pk, fetch, seed, 20, point_of_trust=(5, sig[5]), window=window)
            many = trusted_previous_signature_segments(mv, pk, fetch, seed, 20, point_of_trust=(5, sig[5]),
                                                       window=window)
            assert many == one == (sig[19], (19, sig[19]))
            bad = dict(sig)
            bad[10] = sig[11]
            rounds = []
            for ver in (v, mv):
                with pytest.raises(VerifyError) as ei:
                    trusted_previous_signature_segments(ver, pk, lambda lo, hi: [bad[r] for r in range(lo, hi + 1)],
                                                        seed, 20, point_of_trust=(5, sig[5]), window=window)
                rounds.append(ei.value.round)
            assert rounds == [10, 10]
    finally:
        mv.close()
