"""dgpu_verify_segment_shard_device and dgpu_rlc_root_segment_device: one
shard of a linked segment on one context, the previous signature of its first
item a one-record halo in device memory (kernels.cuh msg_src_halo).

Defining property: verdict bits, reasons and randomness equal
dgpu_verify_beacons_device on the records rounds[i] = first_round + i,
prev[0] = halo, prev_len[0] = *d_halo_len, prev[i] = sigs[i - 1], prev_len
likewise, prev_stride = sig_stride (`segment_helpers.shifted`), under the same key, mode and
RLC seed -- and so rows c.. of dgpu_verify_segment_device on the whole
segment when the halo is record c - 1.  Wherever a test compares with those
calls it also states the expected verdicts by construction.  The over-long
and garbage halos are inputs the contract defines.  Marked gpu."""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import open_ctx
from segment_helpers import (DEFAULTS, check_randomness, corrupted_chain, dev, explicit_device, golden_run,
                             halo_tensor, read_verdicts, segment_device, shard_device, to_dev, u8, verdict_tensors)

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(None)


# ------------------------------------------------------------------ 1. golden chains
def test_golden_chained_chain_every_cut(gpu_ctx):
    """Rounds [c, 24) with halo = record c - 1, for every cut: rows c.. of the
    whole segment (all valid: the fixture links from its genesis seed)."""
    _, code, pk, first, sigs, sig_len, seed = golden_run("chained")
    n = len(sig_len)
    assert n == 24
    _, whole, whole_rand = segment_device(gpu_ctx, code, pk, first, sigs, sig_len, seed)
    assert whole.tolist() == [0] * n
    check_randomness(whole_rand, sigs, sig_len, whole)
    for c in range(1, n):
        s, ln, halo = sigs[c:].copy(), sig_len[c:].copy(), bytes(sigs[c - 1])
        rc, reason, rand = shard_device(gpu_ctx, code, pk, first + c, s, ln, halo, 96)
        assert rc == 0 and reason.tolist() == whole[c:].tolist(), c
        assert np.array_equal(rand, whole_rand[c:]), c
        assert reason.tolist() == explicit_device(gpu_ctx, code, pk, first + c, s, ln, halo, 96).tolist(), c


@pytest.mark.parametrize("name", ["unchained", "on_g1", "g1_rfc9380"])
def test_golden_unchained_chains_never_touch_the_halo(gpu_ctx, name):
    """NULL halo pointers: these schemes ignore previous signatures."""
    _, code, pk, first, sigs, sig_len, seed = golden_run(name)
    n, c = len(sig_len), len(sig_len) // 3
    _, whole, whole_rand = segment_device(gpu_ctx, code, pk, first, sigs, sig_len, seed)
    assert whole.tolist() == [0] * n
    s, ln = sigs[c:].copy(), sig_len[c:].copy()
    rc, reason, rand = shard_device(gpu_ctx, code, pk, first + c, s, ln, b"", 0, null_halo=True)
    assert rc == 0 and reason.tolist() == whole[c:].tolist()
    assert np.array_equal(rand, whole_rand[c:])
    check_randomness(rand, s, ln, reason)
    assert reason.tolist() == explicit_device(gpu_ctx, code, pk, first + c, s, ln, b"", 0).tolist()


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
        want = explicit_device(gpu_ctx, code, c.pk, 1 + cut, s, ln, halo, halo_len)
        assert want.tolist() == [first_reason] + rest, halo_len  # by construction
        rc, reason, rand = shard_device(gpu_ctx, code, c.pk, 1 + cut, s, ln, halo, halo_len)
        assert rc == 0 and reason.tolist() == want.tolist(), halo_len
        check_randomness(rand, s, ln, reason)


def test_rlc_mode_below_the_threshold_runs_per_round(chain9):
    """Library defaults (DGPU_RLC_MIN = 131072): a 5-round RLC call takes the per-round path."""
    from drand_amd import _lib
    code, c, cut = _lib.SCHEME_CHAINED, chain9, 4
    s, ln = c.sigs[cut:].copy(), c.sig_len[cut:].copy()
    ctx = open_ctx(dict(DEFAULTS))
    with contextlib.closing(ctx):
        for halo, want in ((bytes(c.sigs[cut - 1]), [0] * 5), (bytes(c.sigs[0]), [_lib.REASON_PAIRING] + [0] * 4)):
            rc, reason, _ = shard_device(ctx, code, c.pk, 1 + cut, s, ln, halo, 96, _lib.MODE_RLC, 77)
            assert rc == 0 and reason.tolist() == want


def test_halo_is_read_in_stream_order(gpu_ctx, chain9):
    """The halo tensor holds garbage; the right record is copied into it on
    the call's stream immediately before the call, with no synchronise in
    between: item 0 verifies, so the kernels read the halo after the copy."""
    import torch
    from drand_amd import _lib, calls
    code, c, cut = _lib.SCHEME_CHAINED, chain9, 4
    s, ln = c.sigs[cut:].copy(), c.sig_len[cut:].copy()
    n, stride = s.shape
    ts, tl = to_dev(s), to_dev(ln)
    right, right_len = halo_tensor(bytes(c.sigs[cut - 1]), 96, stride)
    halo = torch.full((stride,), 0x5A, dtype=torch.uint8, device=dev())
    halo_len = torch.full((1,), 7, dtype=torch.int32, device=dev())
    bits, reason, _ = verdict_tensors(n, rand=False)
    stream = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()  # the garbage and the inputs are in place
    with torch.cuda.stream(stream):
        halo.copy_(right, non_blocking=True)
        halo_len.copy_(right_len, non_blocking=True)
        calls.verify_segment_shard_device(gpu_ctx, code, c.pk, 1 + cut, ts, tl, halo, halo_len, _lib.MODE_PER_ROUND, 0,
                                          bits, reason, None, stream)
    stream.synchronize()
    assert reason.cpu().numpy().tolist() == [0] * n


# ------------------------------------------------------------------ 3. RLC mode, mid-segment shard
@pytest.fixture(scope="module")
def chain3001():
    from drand_amd import _lib
    c, invalid, _ = corrupted_chain(41, 3001, _lib.SCHEME_CHAINED)
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
    rc, per_round, rand = shard_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len)
    assert rc == 0 and np.array_equal(per_round != 0, expect[CUT:])  # by construction
    check_randomness(rand, s, ln, per_round)
    rs = 0x5EED0000 + len(ln)
    rc, rlc, rand = shard_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len, _lib.MODE_RLC, rs)
    assert rc == 0 and np.array_equal(rlc, per_round)
    check_randomness(rand, s, ln, rlc)
    want = explicit_device(gpu_ctx, code, c.pk, first + CUT, s, ln, halo, halo_len, _lib.MODE_RLC, rs)
    assert np.array_equal(rlc, want)


# ------------------------------------------------------------------ 4. per-rank protocol, two contexts of one GPU
def _root_segment(ctx, code, pk, first_round, ts, tl, lo, hi, seed, halo, rlc_seed, root):
    from drand_amd import calls
    calls.rlc_root_segment_device(ctx, code, pk, first_round + lo, ts[lo:hi], tl[lo:hi], seed, *halo, rlc_seed, root)


def test_per_rank_protocol_on_two_contexts(gpu_ctx, chain3001):
    """Seed form on the first context, halo form on the second (its halo: the
    record before its shard, where it lies in device memory); the roots
    concatenated by a device copy; the finish step on each.  The reasons equal
    the single-context segment call's; the node fails (segment starts and
    corruptions in both shards), so each shard descends."""
    import torch
    from drand_amd import _lib, calls
    from drand_amd.dist import rank_seed
    code = _lib.SCHEME_CHAINED
    c, expect = chain3001
    n = len(c)
    first, link = int(c.rounds[0]), bytes(c.prev[0, :c.prev_len[0]])
    _, single, _ = segment_device(gpu_ctx, code, c.pk, first, c.sigs, c.sig_len, link)
    assert np.array_equal(single != 0, expect)  # by construction
    assert expect[:CUT].any() and expect[CUT:].any()
    rb = calls.rlc_root_bytes(gpu_ctx, code)
    ts, tl = to_dev(c.sigs), to_dev(c.sig_len)
    halo = (ts[CUT - 1], tl[CUT - 1:CUT])  # views: the record where it lies
    second = open_ctx({})
    with contextlib.closing(second):
        ranks = [(gpu_ctx, 0, CUT, (None, None)), (second, CUT, n, halo)]
        roots = [torch.zeros(rb, dtype=torch.uint8, device=dev()) for _ in ranks]
        torch.cuda.synchronize()
        for k, (ctx, lo, hi, hp) in enumerate(ranks):
            _root_segment(ctx, code, c.pk, first, ts, tl, lo, hi, link, hp, rank_seed(1000, k, 2), roots[k])
        all_roots = torch.cat(roots)  # (the NULL stream: ordered after both root calls)
        got = []
        for ctx, lo, hi, _ in ranks:
            bits, reason, _ = verdict_tensors(hi - lo, rand=False)
            calls.rlc_finish_device(ctx, 2, all_roots, bits, reason)
            torch.cuda.synchronize()
            got.append(read_verdicts(bits, reason)[1])
        assert np.array_equal(np.concatenate(got), single)
        # any other verify call on the context cancels the pending root
        _root_segment(second, code, c.pk, first, ts, tl, CUT, n, link, halo, 5, roots[1])
        rc, _, _ = shard_device(second, code, c.pk, first + CUT, c.sigs[CUT:CUT + 8].copy(), c.sig_len[CUT:CUT + 8].copy(),
                                 bytes(c.sigs[CUT - 1]), 96)
        assert rc == 0
        bits = torch.zeros((n - CUT + 7) // 8, dtype=torch.uint8, device=dev())
        rc = second.lib.dgpu_rlc_finish_device(second.handle, 2, all_roots.data_ptr(), bits.data_ptr(), None, NULL)
        assert rc == _lib.DGPU_EINVAL and b"no pending" in second.lib.dgpu_last_error()


# ------------------------------------------------------------------ 5. argument errors, empty shard
def test_argument_errors_and_empty_shard(gpu_ctx, chain9):
    import torch
    from drand_amd import _lib, calls
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    code, c = _lib.SCHEME_CHAINED, chain9
    pkb = u8(c.pk)
    s, ln = c.sigs[4:].copy(), c.sig_len[4:].copy()
    ts, tl = to_dev(s), to_dev(ln)
    th, thl = halo_tensor(bytes(c.sigs[3]), 96, 96)
    bits = torch.zeros(1, dtype=torch.uint8, device=dev())
    rb = calls.rlc_root_bytes(gpu_ctx, code)
    root = torch.zeros(rb, dtype=torch.uint8, device=dev())
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
    junk = u8(bytes(97))
    rc = lib.dgpu_rlc_root_segment_device(h, code, _lib.ptr(pkb), pkb.size, 5, 5, ts.data_ptr(), 96, tl.data_ptr(),
                                          _lib.ptr(junk), 97, None, None, 1, root.data_ptr(), NULL)
    assert rc == _lib.DGPU_EINVAL and b"seed_prev_len" in lib.dgpu_last_error()
    # n = 0: a no-op that accepts NULL pointers, in both modes; the root call yields the identity root
    for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
        assert lib.dgpu_verify_segment_shard_device(h, code, _lib.ptr(pkb), pkb.size, 5, 0, None, 96, None, None, None,
                                                    mode, 7, None, None, None, NULL) == 0
    ident = torch.full((rb,), 0xEE, dtype=torch.uint8, device=dev())
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
