"""dgpu_verify_segment_shard_device and dgpu_rlc_root_segment_device: one
shard of a linked segment on one context, the previous signature of its first
item a one-record halo in device memory (kernels.cuh msg_src_halo).

Defining property: verdict bits, reasons and randomness equal
dgpu_verify_beacons_device on the records rounds[i] = first_round + i,
prev[0] = halo, prev_len[0] = *d_halo_len, prev[i] = sigs[i - 1], prev_len
likewise, prev_stride = sig_stride (`_shifted`), under the same key, mode and
RLC seed -- and so rows c.. of dgpu_verify_segment_device on the whole
segment when the halo is record c - 1.  Wherever a test compares with those
calls it also states the expected verdicts by construction.  The over-long
and garbage halos are inputs the contract defines.  Marked gpu."""
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
NULL = ctypes.c_void_p(None)


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _halo_tensor(halo, halo_len, stride):
    """The halo record as the call reads it: min(halo_len, stride) bytes of
    `halo` at the front of a stride-byte record (the rest 0xA5: bytes past the
    length must not matter), and the length, as two device tensors."""
    rec = np.full(stride, 0xA5, dtype=np.uint8)
    held = min(halo_len, stride, len(halo))
    rec[:held] = _u8(halo)[:held]
    return _to_dev(rec), _to_dev(np.array([halo_len], dtype=np.uint32).view(np.int32))


def _shard_device(ctx, code, pk, first_round, sigs, sig_len, halo, halo_len, mode=0, rlc_seed=0, null_halo=False):
    """(rc, reasons, randomness) of the shard call on the NULL stream."""
    import torch
    from drand_amd import _lib
    n, stride = sigs.shape
    ts, tl = _to_dev(sigs), _to_dev(sig_len.view(np.int32))
    th, thl = (None, None) if null_halo else _halo_tensor(halo, halo_len, stride)
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=_dev())
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=_dev())
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=_dev())
    pkb = _u8(pk)
    torch.cuda.synchronize()
    rc = ctx.lib.dgpu_verify_segment_shard_device(
        ctx.handle, code, _lib.ptr(pkb), pkb.size, first_round, n, ts.data_ptr(), stride, tl.data_ptr(),
        None if null_halo else th.data_ptr(), None if null_halo else thl.data_ptr(), mode, rlc_seed, bits.data_ptr(),
        reason.data_ptr(), out.data_ptr(), NULL)
    _lib.check(ctx.lib.dgpu_synchronize(ctx.handle), ctx.lib)
    torch.cuda.synchronize()
    r = reason.cpu().numpy()
    if rc == 0:
        assert np.array_equal(np.unpackbits(bits.cpu().numpy(), bitorder="little")[:n].astype(bool), r == 0)
    return rc, r, out.cpu().numpy()


def _shifted(first_round, sigs, sig_len, halo, halo_len):
    """The explicit records of the defining property."""
    n, stride = sigs.shape
    rounds = (np.uint64(first_round) + np.arange(n, dtype=np.uint64)).astype(np.uint64)
    prev = np.zeros((n, stride), dtype=np.uint8)
    prev_len = np.zeros(n, dtype=np.uint32)
    held = min(halo_len, stride, len(halo))
    prev[0, :held] = _u8(halo)[:held]
    prev_len[0] = halo_len
    prev[1:] = sigs[:-1]
    prev_len[1:] = sig_len[:-1]
    return rounds, prev, prev_len


def _explicit_device(ctx, code, pk, first_round, sigs, sig_len, halo, halo_len, mode=0, rlc_seed=0):
    """dgpu_verify_beacons_device on the shifted records: the reference of the defining property."""
    import torch
    from drand_amd import _lib
    n = sigs.shape[0]
    rounds, prev, prev_len = _shifted(first_round, sigs, sig_len, halo, halo_len)
    t = [_to_dev(a) for a in (rounds.view(np.int64), sigs, sig_len.view(np.int32), prev, prev_len.view(np.int32))]
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=_dev())
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=_dev())
    pkb = _u8(pk)
    torch.cuda.synchronize()
    _lib.check(ctx.lib.dgpu_verify_beacons_device(ctx.handle, code, _lib.ptr(pkb), pkb.size, n, t[0].data_ptr(),
                                                  t[1].data_ptr(), sigs.shape[1], t[2].data_ptr(), t[3].data_ptr(),
                                                  prev.shape[1], t[4].data_ptr(), mode, rlc_seed, bits.data_ptr(),
                                                  reason.data_ptr(), NULL), ctx.lib)
    torch.cuda.synchronize()
    return reason.cpu().numpy()


def _segment_device(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0):
    """(reasons, randomness) of dgpu_verify_segment_device on a whole segment."""
    import torch
    from drand_amd import _lib
    n = sigs.shape[0]
    ts, tl = _to_dev(sigs), _to_dev(sig_len.view(np.int32))
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=_dev())
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=_dev())
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=_dev())
    pkb, sd = _u8(pk), _u8(seed)
    torch.cuda.synchronize()
    _lib.check(ctx.lib.dgpu_verify_segment_device(ctx.handle, code, _lib.ptr(pkb), pkb.size, first_round, n,
                                                  ts.data_ptr(), sigs.shape[1], tl.data_ptr(),
                                                  _lib.ptr(sd) if sd.size else None, sd.size, mode, rlc_seed,
                                                  bits.data_ptr(), reason.data_ptr(), out.data_ptr(), NULL), ctx.lib)
    torch.cuda.synchronize()
    return reason.cpu().numpy(), out.cpu().numpy()


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
    return code, bytes.fromhex(g["pk"]), rs[0]["round"], sigs, sig_len, bytes.fromhex(rs[0]["prev"])


# ------------------------------------------------------------------ 1. golden chains
def test_golden_chained_chain_every_cut(gpu_ctx):
    """Rounds [c, 24) with halo = record c - 1, for every cut: rows c.. of the
    whole segment (all valid: the fixture links from its genesis seed)."""
    code, pk, first, sigs, sig_len, seed = _golden_run("chained")
    n = len(sig_len)
    assert n == 24
    whole, whole_rand = _segment_device(gpu_ctx, code, pk, first, sigs, sig_len, seed)
    assert whole.tolist() == [0] * n
    _check_randomness(whole_rand, sigs, sig_len, whole)
    for c in range(1, n):
        s, ln, halo = sigs[c:].copy(), sig_len[c:].copy(), bytes(sigs[c - 1])
        rc, reason, rand = _shard_device(gpu_ctx, code, pk, first + c, s, ln, halo, 96)
        assert rc == 0 and reason.tolist() == whole[c:].tolist(), c
        assert np.array_equal(rand, whole_rand[c:]), c
        assert reason.tolist() == _explicit_device(gpu_ctx, code, pk, first + c, s, ln, halo, 96).tolist(), c


@pytest.mark.parametrize("name", ["unchained", "on_g1", "g1_rfc9380"])
def test_golden_unchained_chains_never_touch_the_halo(gpu_ctx, name):
    """NULL halo pointers: these schemes ignore previous signatures."""
    code, pk, first, sigs, sig_len, seed = _golden_run(name)
    n, c = len(sig_len), len(sig_len) // 3
    whole, whole_rand = _segment_device(gpu_ctx, code, pk, first, sigs, sig_len, seed)
    assert whole.tolist() == [0] * n
    s, ln = sigs[c:].copy(), sig_len[c:].copy()
    rc, reason, rand = _shard_device(gpu_ctx, code, pk, first + c, s, ln, b"", 0, null_halo=True)
    assert rc == 0 and reason.tolist() == whole[c:].tolist()
    assert np.array_equal(rand, whole_rand[c:])
    _check_randomness(rand, s, ln, reason)
    assert reason.tolist() == _explicit_device(gpu_ctx, code, pk, first + c, s, ln, b"", 0).tolist()


# ------------------------------------------------------------------ 2. halo cases
@pytest.fixture(scope="module")
def chain9():
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    return make_chain(321, 9, _lib.SCHEME_CHAINED, seg_len=9)


def test_halo_cases(gpu_ctx, chain9):
    """Rounds 5..9 of a 9-round chain (first_round 1), halo = round 4's record."""
    from drand_amd import _lib
    code, c, cut = _lib.SCHEME_CHAINED, chain9, 4
    s, ln, right = c.sigs[cut:].copy(), c.sig_len[cut:].copy(), bytes(c.sigs[cut - 1])
    stride, rest = s.shape[1], [0] * (9 - cut - 1)
    flipped = right[:40] + bytes([right[40] ^ 0x08]) + right[41:]
    cases = [(right, 96, 0),
             (flipped, 96, _lib.REASON_PAIRING),  # one flipped halo byte: only item 0 fails
             (right, 0, _lib.REASON_PAIRING), (right, 48, _lib.REASON_PAIRING), (right, 95, _lib.REASON_PAIRING),
             (right, stride + 4, _lib.REASON_DECODE)]  # over-long: a bad record, the rest unaffected
    for halo, halo_len, first_reason in cases:
        want = _explicit_device(gpu_ctx, code, c.pk, 1 + cut, s, ln, halo, halo_len)
        assert want.tolist() == [first_reason] + rest, halo_len  # by construction
        rc, reason, rand = _shard_device(gpu_ctx, code, c.pk, 1 + cut, s, ln, halo, halo_len)
        assert rc == 0 and reason.tolist() == want.tolist(), halo_len
        _check_randomness(rand, s, ln, reason)


def test_rlc_mode_below_the_threshold_runs_per_round(chain9):
    """Library defaults (DGPU_RLC_MIN = 131072): a 5-round RLC call takes the per-round path."""
    from drand_amd import _lib
    code, c, cut = _lib.SCHEME_CHAINED, chain9, 4
    s, ln = c.sigs[cut:].copy(), c.sig_len[cut:].copy()
    ctx = open_ctx(dict(DEFAULTS))
    with contextlib.closing(ctx):
        for halo, want in ((bytes(c.sigs[cut - 1]), [0] * 5), (bytes(c.sigs[0]), [_lib.REASON_PAIRING] + [0] * 4)):
            rc, reason, _ = _shard_device(ctx, code, c.pk, 1 + cut, s, ln, halo, 96, _lib.MODE_RLC, 77)
            assert rc == 0 and reason.tolist() == want


def test_halo_is_read_in_stream_order(gpu_ctx, chain9):
    """The halo tensor holds garbage; the right record is copied into it on
    the call's stream immediately before the call, with no synchronise in
    between: item 0 verifies, so the kernels read the halo after the copy."""
    import torch
    from drand_amd import _lib
    code, c, cut = _lib.SCHEME_CHAINED, chain9, 4
    s, ln = c.sigs[cut:].copy(), c.sig_len[cut:].copy()
    n, stride = s.shape
    ts, tl = _to_dev(s), _to_dev(ln.view(np.int32))
    right, right_len = _halo_tensor(bytes(c.sigs[cut - 1]), 96, stride)
    halo = torch.full((stride,), 0x5A, dtype=torch.uint8, device=_dev())
    halo_len = torch.full((1,), 7, dtype=torch.int32, device=_dev())
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=_dev())
    reason = torch.full((n,), 0xEE, dtype=torch.uint8, device=_dev())
    pkb = _u8(c.pk)
    stream = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()  # the garbage and the inputs are in place
    with torch.cuda.stream(stream):
        halo.copy_(right, non_blocking=True)
        halo_len.copy_(right_len, non_blocking=True)
        rc = gpu_ctx.lib.dgpu_verify_segment_shard_device(
            gpu_ctx.handle, code, _lib.ptr(pkb), pkb.size, 1 + cut, n, ts.data_ptr(), stride, tl.data_ptr(),
            halo.data_ptr(), halo_len.data_ptr(), _lib.MODE_PER_ROUND, 0, bits.data_ptr(), reason.data_ptr(), None,
            ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0
    stream.synchronize()
    assert reason.cpu().numpy().tolist() == [0] * n


# ------------------------------------------------------------------ 3. RLC mode, mid-segment shard
def _corrupted_segmented_chain(seed, n, code):
    """tests/test_gpu_segment.py's chain: 64-round generator segments, whose
    starts fail in the linked view by construction, every corruption kind the
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
        invalid |= set(range(64, n, 64))  # generator-segment starts: signed over a 32-byte seed
    return c, invalid


@pytest.fixture(scope="module")
def chain3001():
    from drand_amd import _lib
    c, invalid = _corrupted_segmented_chain(41, 3001, _lib.SCHEME_CHAINED)
    expect = np.zeros(len(c), dtype=bool)
    expect[sorted(invalid)] = True
    return c, expect


CUT = 24 * 64 + 40  # the shard starts 40 rounds into a generator segment


def test_rlc_shard_starting_mid_segment(gpu_ctx, chain3001):
    from drand_amd import _lib
    code = _lib.SCHEME_CHAINED
    c, expect = chain3001
    assert CUT % 64 == 40
    first = int(c.rounds[0])
    s, ln = c.sigs[CUT:].copy(), c.sig_len[CUT:].copy()
    halo, halo_len = bytes(c.sigs[CUT - 1]), int(c.sig_len[CUT - 1])
    rc, per_round, rand = _shard_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len)
    assert rc == 0 and np.array_equal(per_round != 0, expect[CUT:])  # by construction
    _check_randomness(rand, s, ln, per_round)
    rs = 0x5EED0000 + len(ln)
    rc, rlc, rand = _shard_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len, _lib.MODE_RLC, rs)
    assert rc == 0 and np.array_equal(rlc, per_round)
    _check_randomness(rand, s, ln, rlc)
    want = _explicit_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len, _lib.MODE_RLC, rs)
    assert np.array_equal(rlc, want)


# ------------------------------------------------------------------ 4. per-rank protocol, two contexts of one GPU
def _root_segment(ctx, code, pk, first_round, ts, tl, lo, hi, stride, seed, halo_ptrs, rlc_seed, root):
    from drand_amd import _lib
    pkb, sd = _u8(pk), _u8(seed)
    return ctx.lib.dgpu_rlc_root_segment_device(
        ctx.handle, code, _lib.ptr(pkb), pkb.size, first_round + lo, hi - lo, ts.data_ptr() + lo * stride, stride,
        tl.data_ptr() + 4 * lo, _lib.ptr(sd) if sd.size else None, sd.size, halo_ptrs[0], halo_ptrs[1], rlc_seed,
        root.data_ptr(), NULL)


def test_per_rank_protocol_on_two_contexts(gpu_ctx, chain3001):
    """Seed form on the first context, halo form on the second (its halo: the
    record before its shard, where it lies in device memory); the roots
    concatenated by a device copy; the finish step on each.  The reasons equal
    the single-context segment call's; the node fails (segment starts and
    corruptions in both shards), so each shard descends."""
    import torch
    from drand_amd import _lib
    from drand_amd.dist import rank_seed
    code = _lib.SCHEME_CHAINED
    c, expect = chain3001
    n, stride = c.sigs.shape
    first, link = int(c.rounds[0]), bytes(c.prev[0, :c.prev_len[0]])
    single, _ = _segment_device(gpu_ctx, code, c.pk, first, c.sigs, c.sig_len, link)
    assert np.array_equal(single != 0, expect)  # by construction
    assert expect[:CUT].any() and expect[CUT:].any()
    rb = gpu_ctx.lib.dgpu_rlc_root_bytes(code)
    ts, tl = _to_dev(c.sigs), _to_dev(c.sig_len.view(np.int32))
    halo_ptrs = (ts.data_ptr() + (CUT - 1) * stride, tl.data_ptr() + 4 * (CUT - 1))
    second = open_ctx({})
    with contextlib.closing(second):
        ranks = [(gpu_ctx, 0, CUT, (None, None)), (second, CUT, n, halo_ptrs)]
        roots = [torch.zeros(rb, dtype=torch.uint8, device=_dev()) for _ in ranks]
        torch.cuda.synchronize()
        for k, (ctx, lo, hi, hp) in enumerate(ranks):
            rc = _root_segment(ctx, code, c.pk, first, ts, tl, lo, hi, stride, link, hp, rank_seed(1000, k, 2), roots[k])
            assert rc == 0, ctx.lib.dgpu_last_error()
        all_roots = torch.cat(roots)  # (the NULL stream: ordered after both root calls)
        got = []
        for ctx, lo, hi, _ in ranks:
            bits = torch.zeros((hi - lo + 7) // 8, dtype=torch.uint8, device=_dev())
            reason = torch.full((hi - lo,), 0xEE, dtype=torch.uint8, device=_dev())
            _lib.check(ctx.lib.dgpu_rlc_finish_device(ctx.handle, 2, all_roots.data_ptr(), bits.data_ptr(),
                                                      reason.data_ptr(), NULL), ctx.lib)
            torch.cuda.synchronize()
            r = reason.cpu().numpy()
            assert np.array_equal(np.unpackbits(bits.cpu().numpy(), bitorder="little")[:hi - lo].astype(bool), r == 0)
            got.append(r)
        assert np.array_equal(np.concatenate(got), single)
        # any other verify call on the context cancels the pending root
        rc = _root_segment(second, code, c.pk, first, ts, tl, CUT, n, stride, link, halo_ptrs, 5, roots[1])
        assert rc == 0
        rc, _, _ = _shard_device(second, code, c.pk, first + CUT, c.sigs[CUT:CUT + 8].copy(), c.sig_len[CUT:CUT + 8].copy(),
                                 bytes(c.sigs[CUT - 1]), 96)
        assert rc == 0
        bits = torch.zeros((n - CUT + 7) // 8, dtype=torch.uint8, device=_dev())
        rc = second.lib.dgpu_rlc_finish_device(second.handle, 2, all_roots.data_ptr(), bits.data_ptr(), None, NULL)
        assert rc == _lib.DGPU_EINVAL and b"no pending" in second.lib.dgpu_last_error()


# ------------------------------------------------------------------ 5. argument errors, empty shard
def test_argument_errors_and_empty_shard(gpu_ctx, chain9):
    import torch
    from drand_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    code, c = _lib.SCHEME_CHAINED, chain9
    pkb = _u8(c.pk)
    s, ln = c.sigs[4:].copy(), c.sig_len[4:].copy()
    ts, tl = _to_dev(s), _to_dev(ln.view(np.int32))
    th, thl = _halo_tensor(bytes(c.sigs[3]), 96, 96)
    bits = torch.zeros(1, dtype=torch.uint8, device=_dev())
    rb = lib.dgpu_rlc_root_bytes(code)
    root = torch.zeros(rb, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()

    def shard(first, n, halo, halo_len):
        return lib.dgpu_verify_segment_shard_device(h, code, _lib.ptr(pkb), pkb.size, first, n, ts.data_ptr(), 96,
                                                    tl.data_ptr(), halo, halo_len, 0, 0, bits.data_ptr(), None, None,
                                                    NULL)
    # a chained shard needs both halo pointers
    assert shard(5, 5, None, thl.data_ptr()) == _lib.DGPU_EINVAL and b"halo" in lib.dgpu_last_error()
    assert shard(5, 5, th.data_ptr(), None) == _lib.DGPU_EINVAL and b"halo" in lib.dgpu_last_error()
    # first_round + n - 1 must fit 64 bits
    assert shard(2**64 - 4, 5, th.data_ptr(), thl.data_ptr()) == _lib.DGPU_EINVAL and b"overflow" in lib.dgpu_last_error()
    # halo form of the root call: d_halo without d_halo_len
    rc = lib.dgpu_rlc_root_segment_device(h, code, _lib.ptr(pkb), pkb.size, 5, 5, ts.data_ptr(), 96, tl.data_ptr(), None, 0,
                                          th.data_ptr(), None, 1, root.data_ptr(), NULL)
    assert rc == _lib.DGPU_EINVAL and b"halo" in lib.dgpu_last_error()
    # seed form: the seed's own bound
    junk = _u8(bytes(97))
    rc = lib.dgpu_rlc_root_segment_device(h, code, _lib.ptr(pkb), pkb.size, 5, 5, ts.data_ptr(), 96, tl.data_ptr(),
                                          _lib.ptr(junk), 97, None, None, 1, root.data_ptr(), NULL)
    assert rc == _lib.DGPU_EINVAL and b"seed_prev_len" in lib.dgpu_last_error()
    # n = 0: a no-op that accepts NULL pointers, in both modes; the root call yields the identity root
    for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
        assert lib.dgpu_verify_segment_shard_device(h, code, _lib.ptr(pkb), pkb.size, 5, 0, None, 96, None, None, None,
                                                    mode, 7, None, None, None, NULL) == 0
    ident = torch.full((rb,), 0xEE, dtype=torch.uint8, device=_dev())
    _lib.check(lib.dgpu_rlc_root_device(h, code, _lib.ptr(pkb), pkb.size, 0, None, None, 96, None, None, 96, None, 3,
                                        ident.data_ptr(), NULL), lib)
    for halo in (None, th.data_ptr()):
        root.fill_(0xEE)
        torch.cuda.synchronize()
        _lib.check(lib.dgpu_rlc_root_segment_device(h, code, _lib.ptr(pkb), pkb.size, 5, 0, None, 96, None, None, 0, halo,
                                                    None if halo is None else thl.data_ptr(), 3, root.data_ptr(), NULL),
                   lib)
        torch.cuda.synchronize()
        assert torch.equal(root, ident)
    # the context still serves
    assert shard(5, 5, th.data_ptr(), thl.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(bits.cpu()[0]) == 0b11111
