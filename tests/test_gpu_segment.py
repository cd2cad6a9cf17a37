"""dgpu_verify_segment / dgpu_verify_segment_device: a linked chain segment
verified from its signatures alone (the walk of client/verify.go:118-178),
with each verified round's randomness (client/verify.go:207).

Defining property: verdict bits and reasons equal dgpu_verify_beacons_device
on the records rounds[i] = first_round + i, prev[0] = seed, prev[i] =
sigs[i - 1], prev_len likewise, prev_stride = sig_stride (`segment_helpers.shifted`), under
the same key, mode and RLC seed -- in the host form and the device form.
Wherever a test compares with that call it also states the expected verdicts
by construction.  Marked gpu."""
import contextlib

import numpy as np
import pytest

from conftest import load_golden, open_ctx
from segment_helpers import (DEFAULTS, GOLDEN, check_randomness, corrupted_chain, explicit_device, golden_run,
                             segment_device, segment_host, u8)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. golden chains
def test_chained_golden_fixture_is_linked_from_the_genesis_seed():
    """(CPU check of the fixture the tests below rely on.)"""
    g = load_golden(GOLDEN["chained"])
    rs = g["rounds"]
    assert len(rs) == 24 and rs[0]["prev"] == g["genesis"]
    assert all(rs[i]["prev"] == rs[i - 1]["sig"] for i in range(1, len(rs)))


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_chain_segments(gpu_ctx, name):
    g, code, pk, first, sigs, sig_len, seed = golden_run(name)
    n = len(sig_len)
    for call in (segment_host, segment_device):
        rc, reason, rand = call(gpu_ctx, code, pk, first, sigs, sig_len, seed)
        assert rc == 0 and reason.tolist() == [0] * n
        check_randomness(rand, sigs, sig_len, reason)
    mid = n // 2
    bad = sigs.copy()
    bad[mid, 5] ^= 0x10
    fails = {mid, mid + 1} if name == "chained" else {mid}
    for call in (segment_host, segment_device):
        rc, reason, rand = call(gpu_ctx, code, pk, first, bad, sig_len, seed)
        assert rc == 0 and set(np.nonzero(reason)[0].tolist()) == fails
        check_randomness(rand, bad, sig_len, reason)
        assert all(bytes(rand[i]) == bytes(32) for i in fails)
        assert all(bytes(rand[i]) != bytes(32) for i in range(n) if i not in fails)


# ------------------------------------------------------------------ 2. small fully linked chains
@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 64, 65])
def test_small_linked_chains(gpu_ctx, n):
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    c = make_chain(300 + n, n, _lib.SCHEME_CHAINED, seg_len=n)
    seed = bytes(c.prev[0, :c.prev_len[0]])
    assert len(seed) == 32
    for call in (segment_host, segment_device):
        rc, reason, rand = call(gpu_ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, seed)
        assert rc == 0 and reason.tolist() == [0] * n
        check_randomness(rand, c.sigs, c.sig_len, reason)
        wrong = bytes([seed[0] ^ 1]) + seed[1:]
        rc, reason, rand = call(gpu_ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, wrong)
        assert rc == 0 and reason.tolist() == [_lib.REASON_PAIRING] + [0] * (n - 1)
        check_randomness(rand, c.sigs, c.sig_len, reason)


def test_seed_lengths_and_argument_errors(gpu_ctx):
    """Seeds of 0, 32 and 96 bytes (the digest's padding takes another path at
    each: 8, 40 and 104 hashed bytes -- one block, one block, two blocks)
    against the explicit call; the two EINVALs; the context serves the next call."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    code = _lib.SCHEME_CHAINED
    c = make_chain(321, 9, code, seg_len=9)
    seed32 = bytes(c.prev[0, :32])
    for seed in (b"", seed32, bytes(c.sigs[3])):
        want = explicit_device(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, seed)
        assert want.tolist() == ([0] * 9 if seed == seed32 else [_lib.REASON_PAIRING] + [0] * 8)
        for call in (segment_host, segment_device):
            rc, reason, _ = call(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, seed)
            assert rc == 0 and reason.tolist() == want.tolist(), len(seed)
    # a chain that really links from a 96-byte seed: rounds 2.. of the chain, seeded by round 1's signature
    for call in (segment_host, segment_device):
        rc, reason, _ = call(gpu_ctx, code, c.pk, 2, c.sigs[1:].copy(), c.sig_len[1:].copy(), bytes(c.sigs[0]))
        assert rc == 0 and reason.tolist() == [0] * 8
    for call in (segment_host, segment_device):
        rc, _, _ = call(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, bytes(97))
        assert rc == _lib.DGPU_EINVAL and b"seed_prev_len" in gpu_ctx.lib.dgpu_last_error()
        rc, _, _ = call(gpu_ctx, code, c.pk, 2**64 - 2, c.sigs[:3].copy(), c.sig_len[:3].copy(), seed32)
        assert rc == _lib.DGPU_EINVAL and b"overflow" in gpu_ctx.lib.dgpu_last_error()
        # 2**64 - 3 .. 2**64 - 1 is the last range that fits; and the context still serves
        rc, reason, _ = call(gpu_ctx, code, c.pk, 2**64 - 3, c.sigs[:3].copy(), c.sig_len[:3].copy(), seed32)
        assert rc == 0 and reason.tolist() == [_lib.REASON_PAIRING] * 3
        rc, reason, _ = call(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, seed32)
        assert rc == 0 and reason.tolist() == [0] * 9


# ------------------------------------------------------------------ 3. equivalence with the explicit call
def _equivalence(ctx, code, n, seed, modes):
    from drand_amd import _lib
    c, invalid, over = corrupted_chain(seed, n, code)
    first = int(c.rounds[0])
    link = bytes(c.prev[0, :c.prev_len[0]])  # segment 0's seed (ignored by the unchained schemes)
    expect = np.zeros(n, dtype=bool)
    expect[sorted(invalid)] = True
    for mode in modes:
        rs = 0x5EED0000 + n if mode == _lib.MODE_RLC else 0
        want = explicit_device(ctx, code, c.pk, first, c.sigs, c.sig_len, link, mode=mode, rlc_seed=rs)
        assert np.array_equal(want != 0, expect)  # every round has an expected verdict, by construction
        assert want[over] == _lib.REASON_DECODE
        if code == _lib.SCHEME_CHAINED:
            assert want[over + 1] == _lib.REASON_DECODE  # the record after the over-long one
        for call in (segment_host, segment_device):
            rc, reason, rand = call(ctx, code, c.pk, first, c.sigs, c.sig_len, link, mode, rs)
            assert rc == 0
            assert np.array_equal(reason, want), (mode, call.__name__, np.nonzero(reason != want)[0][:10])
            check_randomness(rand, c.sigs, c.sig_len, reason)


def test_equivalence_with_explicit_records_chained(gpu_ctx):
    from drand_amd import _lib
    _equivalence(gpu_ctx, _lib.SCHEME_CHAINED, 3001, 41, (_lib.MODE_PER_ROUND, _lib.MODE_RLC))


@pytest.mark.parametrize("code_name", ["SCHEME_UNCHAINED", "SCHEME_UNCHAINED_G1"])
def test_equivalence_with_explicit_records_unchained(gpu_ctx, code_name):
    from drand_amd import _lib
    _equivalence(gpu_ctx, getattr(_lib, code_name), 41, 43, (_lib.MODE_PER_ROUND, _lib.MODE_RLC))


# ------------------------------------------------------------------ 4. across the lane slices
def test_linkage_across_lane_slices(gpu_ctx):
    """n = 262,149 takes the two-lane path (LANE_MIN = 262,144) in slices of
    whole 5-round engine blocks: the second slice starts at round index
    131,075 and its first item reads the last record of the first slice."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    code, n = _lib.SCHEME_CHAINED, 262149
    c = make_chain(77, n, code, seg_len=64)
    link = bytes(c.prev[0, :32])
    starts = set(range(64, n, 64))
    for where in (131074, 131075):
        sigs = c.sigs.copy()
        sigs[where, 0] ^= 0x20  # y sign: a valid point, the wrong signature
        want = explicit_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
        assert set(np.nonzero(want)[0].tolist()) == starts | {where, where + 1}
        rc, reason, _ = segment_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
        assert rc == 0 and np.array_equal(reason, want)
        rc, reason, _ = segment_host(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link, rand=False)
        assert rc == 0 and np.array_equal(reason, want)
        assert _lib.staging_stats(gpu_ctx)[2] == n * (sigs.shape[1] + 4)
    # the caller's buffers are its own again once the host call has returned
    sigs[:] = np.roll(sigs, 1, axis=0)
    want = explicit_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
    assert np.count_nonzero(want) > n - 8  # (rolled by one: every round now carries its predecessor's signature)
    rc, reason, _ = segment_host(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link, rand=False)
    assert rc == 0 and np.array_equal(reason, want)


# ------------------------------------------------------------------ 5. library defaults
def test_segments_at_library_defaults():
    """One context under the shipped thresholds: the small-call latency path
    (n = 9) and RLC mode falling back to per-round below DGPU_RLC_MIN."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    ctx = open_ctx(dict(DEFAULTS))
    with contextlib.closing(ctx):
        c = make_chain(309, 9, _lib.SCHEME_CHAINED, seg_len=9)
        seed = bytes(c.prev[0, :32])
        for call in (segment_host, segment_device):
            rc, reason, rand = call(ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, seed)
            assert rc == 0 and reason.tolist() == [0] * 9
            check_randomness(rand, c.sigs, c.sig_len, reason)
        _equivalence(ctx, _lib.SCHEME_CHAINED, 3001, 41, (_lib.MODE_PER_ROUND, _lib.MODE_RLC))


@pytest.mark.parametrize("mode_name", ["MODE_PER_ROUND", "MODE_RLC"])
def test_randomness_stage_is_profiled_within_max_stages(mode_name):
    """k_randomness has a stage of its own, and the segment pipelines (per
    round; RLC with a failing root, descent and confirmation) stay within
    DGPU_MAX_STAGES (_lib.stage_times raises above it)."""
    from drand_amd import _lib, calls
    from drand_amd.synth import make_chain
    ctx = open_ctx({})
    with contextlib.closing(ctx):
        c = make_chain(311, 200, _lib.SCHEME_CHAINED, seg_len=64)  # segment starts fail: the RLC root fails too
        with calls.profiled(ctx) as stage_times:
            rc, reason, rand = segment_host(ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len,
                                            bytes(c.prev[0, :32]), getattr(_lib, mode_name), 99)
            assert rc == 0 and np.nonzero(reason)[0].tolist() == [64, 128, 192]
            stages = stage_times()
        assert "randomness" in stages and "pack_verdicts" in stages and len(stages) <= _lib.MAX_STAGES
        check_randomness(rand, c.sigs, c.sig_len, reason)


# ------------------------------------------------------------------ 6. empty batch
def test_empty_segment_is_a_no_op(gpu_ctx):
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    for code in (_lib.SCHEME_CHAINED, _lib.SCHEME_UNCHAINED_G1):
        pk = u8(make_chain(72, 2, code, seg_len=2).pk)
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            _lib.check(lib.dgpu_verify_segment(h, code, _lib.ptr(pk), pk.size, 5, 0, None, 96, None, None, 0, mode, 7,
                                               None, None, None), lib)
            _lib.check(lib.dgpu_verify_segment_device(h, code, _lib.ptr(pk), pk.size, 5, 0, None, 96, None, None, 0,
                                                      mode, 7, None, None, None, None), lib)


# ------------------------------------------------------------------ 7. Python mirror
def test_python_verify_segment_and_segment_walk():
    from drand_amd.chain import Beacon, VerifyError, new_verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.sync import trusted_previous_signature, trusted_previous_signature_segments
    g = load_golden(GOLDEN["chained"])
    v = new_verifier(get_scheme_by_id_with_default(g["scheme"]))
    pk = bytes.fromhex(g["pk"])
    beacons = [Beacon(bytes.fromhex(r["prev"]), r["round"], bytes.fromhex(r["sig"])) for r in g["rounds"]]
    sigs = [b.signature for b in beacons]
    for tamper in (None, 11):
        if tamper is not None:
            sigs[tamper] = sigs[tamper][:7] + bytes([sigs[tamper][7] ^ 4]) + sigs[tamper][8:]
            beacons = [Beacon(p, b.round, s) for p, b, s in zip([beacons[0].previous_sig] + sigs[:-1], beacons, sigs)]
        reasons, rand = v.verify_segment(beacons[0].round, sigs, beacons[0].previous_sig, pk)
        assert reasons.tolist() == v.verify_reasons(beacons, pk).tolist()
        assert np.count_nonzero(reasons) == (0 if tamper is None else 2)
        check_randomness(rand, np.stack([u8(s) for s in sigs]), np.full(len(sigs), 96), reasons)
        arr = np.stack([u8(s) for s in sigs])
        r2, none = v.verify_segment(beacons[0].round, arr, beacons[0].previous_sig, pk, randomness=False,
                                    sig_len=np.full(len(sigs), 96, dtype=np.uint32))
        assert none is None and r2.tolist() == reasons.tolist()
    sig = {r["round"]: bytes.fromhex(r["sig"]) for r in g["rounds"]}
    seed = bytes.fromhex(g["genesis"])
    for window in (7, 1 << 14):
        fetch = lambda lo, hi, s=sig: [s[r] for r in range(lo, hi + 1)]
        got = trusted_previous_signature_segments(v, pk, fetch, seed, 20, point_of_trust=(5, sig[5]), window=window)
        assert got == trusted_previous_signature(v, pk, sig.__getitem__, seed, 20, point_of_trust=(5, sig[5]),
                                                 window=window) == (sig[19], (19, sig[19]))
        bad = dict(sig)
        bad[10] = sig[11]
        rounds = []
        for walk, get in ((trusted_previous_signature_segments, lambda lo, hi: [bad[r] for r in range(lo, hi + 1)]),
                          (trusted_previous_signature, bad.__getitem__)):
            with pytest.raises(VerifyError) as ei:
                walk(v, pk, get, seed, 20, point_of_trust=(5, sig[5]), window=window)
            rounds.append(ei.value.round)
        assert rounds == [10, 10]
