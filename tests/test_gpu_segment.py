"""dgpu_verify_segment / dgpu_verify_segment_device: a linked chain segment
verified from its signatures alone (the walk of client/verify.go:118-178),
with each verified round's randomness (client/verify.go:207).

Defining property: verdict bits and reasons equal dgpu_verify_beacons_device
on the records rounds[i] = first_round + i, prev[0] = seed, prev[i] =
sigs[i - 1], prev_len likewise, prev_stride = sig_stride (`_shifted`), under
the same key, mode and RLC seed -- in the host form and the device form.
Wherever a test compares with that call it also states the expected verdicts
by construction.  Marked gpu."""
import contextlib
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden, open_ctx

pytestmark = pytest.mark.gpu

GOLDEN = {"chained": "chain_chained_s1.json", "unchained": "chain_unchained_s1.json",
          "on_g1": "chain_on_g1_s1.json", "g1_rfc9380": "chain_g1_rfc9380_s2.json"}
DEFAULTS = {"DGPU_THR_MIN": "65536", "DGPU_RLC_MIN": "131072", "DGPU_COF_ENGINE_MAX": "16384",
            "DGPU_FE_GS_MAX": "16384"}


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _shifted(first_round, sigs, sig_len, seed):
    """The explicit records of the defining property."""
    n, stride = sigs.shape
    rounds = (np.uint64(first_round) + np.arange(n, dtype=np.uint64)).astype(np.uint64)
    prev = np.zeros((n, stride), dtype=np.uint8)
    prev_len = np.zeros(n, dtype=np.uint32)
    prev[0, :min(len(seed), stride)] = _u8(seed)[:stride]
    prev_len[0] = len(seed)
    prev[1:] = sigs[:-1]
    prev_len[1:] = sig_len[:-1]
    return rounds, prev, prev_len


def _segment_host(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0, rand=True):
    """(rc, reasons, randomness) of the host form; bitmap and reasons must agree."""
    from drand_amd import _lib
    n = sigs.shape[0]
    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
    reason = np.full(n, 0xEE, dtype=np.uint8)
    out = np.full((n, 32), 0xEE, dtype=np.uint8) if rand else None
    pkb, sd = _u8(pk), _u8(seed)
    rc = ctx.lib.dgpu_verify_segment(ctx.handle, code, _lib.ptr(pkb), pkb.size, first_round, n, _lib.ptr(sigs),
                                     sigs.shape[1], _lib.ptr(sig_len), _lib.ptr(sd) if sd.size else None, sd.size,
                                     mode, rlc_seed, _lib.ptr(bits), _lib.ptr(reason), _lib.ptr(out))
    if rc == 0:
        assert np.array_equal(np.unpackbits(bits, bitorder="little")[:n].astype(bool), reason == 0)
    return rc, reason, out


def _segment_device(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0):
    import torch
    from drand_amd import _lib
    dev = torch.device("cuda", 0)
    n = sigs.shape[0]
    ts = torch.from_numpy(sigs).to(dev)
    tl = torch.from_numpy(sig_len.view(np.int32)).to(dev)
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=dev)
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    pkb = _u8(pk)
    sd = bytearray(seed)  # a buffer this function overwrites as soon as the call returns
    sdp = (ctypes.c_uint8 * max(len(sd), 1)).from_buffer(sd) if len(sd) else None
    torch.cuda.synchronize()
    rc = ctx.lib.dgpu_verify_segment_device(ctx.handle, code, _lib.ptr(pkb), pkb.size, first_round, n, ts.data_ptr(),
                                            sigs.shape[1], tl.data_ptr(), sdp, len(sd), mode, rlc_seed,
                                            bits.data_ptr(), reason.data_ptr(), out.data_ptr(), ctypes.c_void_p(None))
    for k in range(len(sd)):  # the seed does not outlive the call in caller memory
        sd[k] = 0xFF
    _lib.check(ctx.lib.dgpu_synchronize(ctx.handle), ctx.lib)
    torch.cuda.synchronize()
    r = reason.cpu().numpy()
    if rc == 0:
        assert np.array_equal(np.unpackbits(bits.cpu().numpy(), bitorder="little")[:n].astype(bool), r == 0)
    return rc, r, out.cpu().numpy()


def _explicit_device(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0):
    """dgpu_verify_beacons_device on the shifted records: the reference of the defining property."""
    import torch
    from drand_amd import _lib
    dev = torch.device("cuda", 0)
    n = sigs.shape[0]
    rounds, prev, prev_len = _shifted(first_round, sigs, sig_len, seed)
    t = [torch.from_numpy(a).to(dev) for a in (rounds.view(np.int64), sigs, sig_len.view(np.int32), prev,
                                               prev_len.view(np.int32))]
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=dev)
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    pkb = _u8(pk)
    torch.cuda.synchronize()
    _lib.check(ctx.lib.dgpu_verify_beacons_device(ctx.handle, code, _lib.ptr(pkb), pkb.size, n, t[0].data_ptr(),
                                                  t[1].data_ptr(), sigs.shape[1], t[2].data_ptr(), t[3].data_ptr(),
                                                  prev.shape[1], t[4].data_ptr(), mode, rlc_seed, bits.data_ptr(),
                                                  reason.data_ptr(), ctypes.c_void_p(None)), ctx.lib)
    torch.cuda.synchronize()
    return reason.cpu().numpy()


def _check_randomness(out, sigs, sig_len, reason):
    """SHA-256 of the signature where the round verifies, zeros elsewhere."""
    for i in range(len(reason)):
        want = hashlib.sha256(bytes(sigs[i, :sig_len[i]])).digest() if reason[i] == 0 else bytes(32)
        assert bytes(out[i]) == want, i


def _golden_run(name):
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    g = load_golden(GOLDEN[name])
    rs = g["rounds"]
    assert [r["round"] for r in rs] == list(range(rs[0]["round"], rs[0]["round"] + len(rs)))
    code = scheme_code(get_scheme_by_id_with_default(g["scheme"]))
    width = len(rs[0]["sig"]) // 2
    sigs = np.stack([_u8(bytes.fromhex(r["sig"])) for r in rs])
    sig_len = np.full(len(rs), width, dtype=np.uint32)
    return g, code, bytes.fromhex(g["pk"]), rs[0]["round"], sigs, sig_len, bytes.fromhex(rs[0]["prev"])


# ------------------------------------------------------------------ 1. golden chains
def test_chained_golden_fixture_is_linked_from_the_genesis_seed():
    """(CPU check of the fixture the tests below rely on.)"""
    g = load_golden(GOLDEN["chained"])
    rs = g["rounds"]
    assert len(rs) == 24 and rs[0]["prev"] == g["genesis"]
    assert all(rs[i]["prev"] == rs[i - 1]["sig"] for i in range(1, len(rs)))


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_chain_segments(gpu_ctx, name):
    g, code, pk, first, sigs, sig_len, seed = _golden_run(name)
    n = len(sig_len)
    for call in (_segment_host, _segment_device):
        rc, reason, rand = call(gpu_ctx, code, pk, first, sigs, sig_len, seed)
        assert rc == 0 and reason.tolist() == [0] * n
        _check_randomness(rand, sigs, sig_len, reason)
    mid = n // 2
    bad = sigs.copy()
    bad[mid, 5] ^= 0x10
    fails = {mid, mid + 1} if name == "chained" else {mid}
    for call in (_segment_host, _segment_device):
        rc, reason, rand = call(gpu_ctx, code, pk, first, bad, sig_len, seed)
        assert rc == 0 and set(np.nonzero(reason)[0].tolist()) == fails
        _check_randomness(rand, bad, sig_len, reason)
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
    for call in (_segment_host, _segment_device):
        rc, reason, rand = call(gpu_ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, seed)
        assert rc == 0 and reason.tolist() == [0] * n
        _check_randomness(rand, c.sigs, c.sig_len, reason)
        wrong = bytes([seed[0] ^ 1]) + seed[1:]
        rc, reason, rand = call(gpu_ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, wrong)
        assert rc == 0 and reason.tolist() == [_lib.REASON_PAIRING] + [0] * (n - 1)
        _check_randomness(rand, c.sigs, c.sig_len, reason)


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
        want = _explicit_device(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, seed)
        assert want.tolist() == ([0] * 9 if seed == seed32 else [_lib.REASON_PAIRING] + [0] * 8)
        for call in (_segment_host, _segment_device):
            rc, reason, _ = call(gpu_ctx, code, c.pk, 1, c.sigs, c.sig_len, seed)
            assert rc == 0 and reason.tolist() == want.tolist(), len(seed)
    # a chain that really links from a 96-byte seed: rounds 2.. of the chain, seeded by round 1's signature
    for call in (_segment_host, _segment_device):
        rc, reason, _ = call(gpu_ctx, code, c.pk, 2, c.sigs[1:].copy(), c.sig_len[1:].copy(), bytes(c.sigs[0]))
        assert rc == 0 and reason.tolist() == [0] * 8
    for call in (_segment_host, _segment_device):
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
def _corrupted_chain(seed, n, code):
    """A chain in 64-round generator segments with every corruption kind the
    linked form has an array for, one sig_len above the stride and one
    sig_len = 0.  Returns (chain, expected-invalid set by construction)."""
    from drand_amd import _lib, synth
    c = synth.make_chain(seed, n, code, seg_len=64)
    kinds = tuple(k for k in synth.ALL_CORRUPTIONS if k != synth.CORRUPT_PREV)
    bad = synth.corrupt(c, seed, rate=4e-3, kinds=kinds)
    free = [i for i in range(3, n - 3) if not any(j in bad for j in range(i - 2, i + 3))]
    over, zero = free[len(free) // 3], free[2 * len(free) // 3]
    c.sig_len[over] = c.sigs.shape[1] + 1
    c.sig_len[zero] = 0
    corrupted = set(bad) | {over, zero}
    invalid = set(corrupted)
    if code == _lib.SCHEME_CHAINED:
        invalid |= {i + 1 for i in corrupted if i + 1 < n}  # the successor hashes the altered record
        invalid |= set(range(64, n, 64))  # generator-segment starts: signed over a 32-byte seed, not the signature before
    return c, invalid, over


def _equivalence(ctx, code, n, seed, modes):
    from drand_amd import _lib
    c, invalid, over = _corrupted_chain(seed, n, code)
    first = int(c.rounds[0])
    link = bytes(c.prev[0, :c.prev_len[0]])  # segment 0's seed (ignored by the unchained schemes)
    expect = np.zeros(n, dtype=bool)
    expect[sorted(invalid)] = True
    for mode in modes:
        rs = 0x5EED0000 + n if mode == _lib.MODE_RLC else 0
        want = _explicit_device(ctx, code, c.pk, first, c.sigs, c.sig_len, link, mode, rs)
        assert np.array_equal(want != 0, expect)  # every round has an expected verdict, by construction
        assert want[over] == _lib.REASON_DECODE
        if code == _lib.SCHEME_CHAINED:
            assert want[over + 1] == _lib.REASON_DECODE  # the record after the over-long one
        for call in (_segment_host, _segment_device):
            rc, reason, rand = call(ctx, code, c.pk, first, c.sigs, c.sig_len, link, mode, rs)
            assert rc == 0
            assert np.array_equal(reason, want), (mode, call.__name__, np.nonzero(reason != want)[0][:10])
            _check_randomness(rand, c.sigs, c.sig_len, reason)


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
        want = _explicit_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
        assert set(np.nonzero(want)[0].tolist()) == starts | {where, where + 1}
        rc, reason, _ = _segment_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
        assert rc == 0 and np.array_equal(reason, want)
        rc, reason, _ = _segment_host(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link, rand=False)
        assert rc == 0 and np.array_equal(reason, want)
        assert _lib.staging_stats(gpu_ctx)[2] == n * (sigs.shape[1] + 4)
    # the caller's buffers are its own again once the host call has returned
    sigs[:] = np.roll(sigs, 1, axis=0)
    want = _explicit_device(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link)
    assert np.count_nonzero(want) > n - 8  # (rolled by one: every round now carries its predecessor's signature)
    rc, reason, _ = _segment_host(gpu_ctx, code, c.pk, 1, sigs, c.sig_len, link, rand=False)
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
        for call in (_segment_host, _segment_device):
            rc, reason, rand = call(ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, seed)
            assert rc == 0 and reason.tolist() == [0] * 9
            _check_randomness(rand, c.sigs, c.sig_len, reason)
        _equivalence(ctx, _lib.SCHEME_CHAINED, 3001, 41, (_lib.MODE_PER_ROUND, _lib.MODE_RLC))


@pytest.mark.parametrize("mode_name", ["MODE_PER_ROUND", "MODE_RLC"])
def test_randomness_stage_is_profiled_within_max_stages(mode_name):
    """k_randomness has a stage of its own, and the segment pipelines (per
    round; RLC with a failing root, descent and confirmation) stay within
    DGPU_MAX_STAGES (_lib.stage_times raises above it)."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    ctx = open_ctx({})
    with contextlib.closing(ctx):
        c = make_chain(311, 200, _lib.SCHEME_CHAINED, seg_len=64)  # segment starts fail: the RLC root fails too
        _lib.check(ctx.lib.dgpu_set_profiling(ctx.handle, 1), ctx.lib)
        rc, reason, rand = _segment_host(ctx, _lib.SCHEME_CHAINED, c.pk, 1, c.sigs, c.sig_len, bytes(c.prev[0, :32]),
                                         getattr(_lib, mode_name), 99)
        assert rc == 0 and np.nonzero(reason)[0].tolist() == [64, 128, 192]
        stages = _lib.stage_times(ctx)
        assert "randomness" in stages and "pack_verdicts" in stages and len(stages) <= _lib.MAX_STAGES
        _check_randomness(rand, c.sigs, c.sig_len, reason)


# ------------------------------------------------------------------ 6. empty batch
def test_empty_segment_is_a_no_op(gpu_ctx):
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    for code in (_lib.SCHEME_CHAINED, _lib.SCHEME_UNCHAINED_G1):
        pk = _u8(make_chain(72, 2, code, seg_len=2).pk)
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            _lib.check(lib.dgpu_verify_segment(h, code, _lib.ptr(pk), pk.size, 5, 0, None, 96, None, None, 0, mode, 7,
                                               None, None, None))
            _lib.check(lib.dgpu_verify_segment_device(h, code, _lib.ptr(pk), pk.size, 5, 0, None, 96, None, None, 0,
                                                      mode, 7, None, None, None, None))


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
        _check_randomness(rand, np.stack([_u8(s) for s in sigs]), np.full(len(sigs), 96), reasons)
        arr = np.stack([_u8(s) for s in sigs])
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
