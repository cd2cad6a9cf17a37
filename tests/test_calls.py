"""drand_amd.calls against a recording stub of the library (no GPU): what
reaches each dgpu_* entry point, whose library a failure's message comes from,
and the bitmap / reasons agreement check of every host-form verify call."""
import ctypes
import types

import numpy as np
import pytest

from drand_amd import _lib, calls
from drand_amd._lib import ptr as P

ARGC = {name: len(args) for name, _, args in _lib.SYMBOLS}
ANY = object()  # an array the function allocates, or its copy of a bytes argument
HANDLE = ctypes.c_void_p(0x1000)
STREAM = types.SimpleNamespace(cuda_stream=0x5000)
PK = bytes(range(48))
SEED = b"\x07" * 32


class StubLib:
    """Every dgpu_* symbol records its arguments, runs `effect` on them and
    returns `rc`; dgpu_last_error is the stub's own."""

    def __init__(self, rc=0, effect=None):
        self.rc, self.effect, self.seen = rc, effect, []

    def dgpu_last_error(self):
        return b"from stub"

    def dgpu_rlc_root_bytes(self, code):
        return 576 if self.rc == 0 else self.rc

    def __getattr__(self, name):
        if not name.startswith("dgpu_"):
            raise AttributeError(name)

        def fn(*args):
            self.seen.append((name, args))
            if self.effect:
                self.effect(name, args)
            return self.rc
        return fn


def stub_ctx(**kw):
    return types.SimpleNamespace(lib=StubLib(**kw), handle=HANDLE)


def arrays(n, stride, long_record=False):
    a = types.SimpleNamespace(n=n, stride=stride)
    a.rounds = np.arange(1, n + 1, dtype=np.uint64)
    a.sigs = np.ones((n, stride), dtype=np.uint8)
    a.sig_len = np.full(n, stride, dtype=np.uint32)
    a.prev = np.ones((n, stride), dtype=np.uint8)
    a.prev_len = np.full(n, stride, dtype=np.uint32)
    if long_record:
        a.sig_len[1] = a.prev_len[1] = stride + 5  # longer than the stride: passed on as it is
    a.msgs = np.ones((n, 32), dtype=np.uint8)
    a.msg_len = np.full(n, 32, dtype=np.uint32)
    a.keys = np.ones(2 * 48, dtype=np.uint8)
    a.idx = np.zeros(n, dtype=np.uint32)
    a.parts = np.ones((n, 2, stride + 2), dtype=np.uint8)
    a.plen = np.full((n, 2), stride + 2, dtype=np.uint32)
    a.base = np.ones(200 * n + 1, dtype=np.uint8)
    a.off = np.arange(n, dtype=np.uint64) * 200
    a.ln = np.full(n, 200, dtype=np.uint32)
    a.rkeys = np.arange(n, dtype=np.uint64)
    a.shares = np.ones(4 * 32, dtype=np.uint8)
    a.sidx = np.zeros((n, 2), dtype=np.uint32)
    # the caller's outputs of the device forms (any array with a pointer stands in for a tensor)
    a.bits, a.reason = np.zeros((n + 7) // 8, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    a.rand, a.root, a.ok = np.zeros((n, 32), dtype=np.uint8), np.zeros(576, dtype=np.uint8), np.zeros(n, np.uint8)
    a.out = np.zeros((n, stride), dtype=np.uint8)
    a.halo, a.halo_len = np.zeros(stride, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    return a


SHAPES = {"n3_stride96": (3, 96), "n3_stride48": (3, 48), "n3_long_record": (3, 96, True), "n0": (0, 96)}
C, M, S = _lib.SCHEME_CHAINED, _lib.MODE_PER_ROUND, 77  # scheme, mode, an explicit RLC seed


def rows_ptrs(a):
    return [P(x) if a.n else None for x in (a.base, a.off, a.ln, a.rkeys)]


def recs(a):  # the record arrays as the calls take them, and what arrives for them (n first)
    return a.rounds, a.sigs, a.sig_len, a.prev, a.prev_len


def recs_args(a):
    return [a.n, P(a.rounds), P(a.sigs), a.stride, P(a.sig_len), P(a.prev), a.stride, P(a.prev_len)]


def raw(a):  # messages and signatures of the raw-message calls
    return a.msgs, a.msg_len, a.sigs, a.sig_len


def raw_args(a):
    return [P(a.msgs), 32, P(a.msg_len), P(a.sigs), a.stride, P(a.sig_len)]


def parts_args(a):  # (a.msgs, a.parts, a.plen) arrives as
    return [a.n, P(a.msgs), 2, P(a.parts), a.stride + 2, P(a.plen)]


def seg_args(a):  # (9, a.sigs, a.sig_len) arrives as
    return [9, a.n, P(a.sigs), a.stride, P(a.sig_len)]


G1 = _lib.SCHEME_G1_RFC9380
# name -> (symbol, call(ctx, a), expected arguments after the handle)
CASES = {
    "set_pubkey": ("dgpu_set_pubkey", lambda c, a: calls.set_pubkey(c, C, PK), lambda a: [C, ANY, 48]),
    "derive_pubkey": ("dgpu_derive_pubkey", lambda c, a: calls.derive_pubkey(c, C, 5), lambda a: [C, ANY, ANY, 48]),
    "derive_pubkey_g1": ("dgpu_derive_pubkey", lambda c, a: calls.derive_pubkey(c, G1, 5), lambda a: [G1, ANY, ANY, 96]),
    "set_group": ("dgpu_set_group", lambda c, a: calls.set_group(c, C, 2, 5, [PK, PK]), lambda a: [2, 5, ANY]),
    "set_group_g1": ("dgpu_set_group_scheme", lambda c, a: calls.set_group(c, G1, 2, 5, [PK + PK] * 2),
                     lambda a: [G1, 2, 5, ANY, 96]),
    "multi_set_group": ("dgpu_multi_set_group", lambda c, a: calls.multi_set_group(c, C, 2, 5, [PK, PK]),
                        lambda a: [2, 5, ANY]),
    "multi_set_group_g1": ("dgpu_multi_set_group_scheme", lambda c, a: calls.multi_set_group(c, G1, 2, 5, [PK + PK] * 2),
                           lambda a: [G1, 2, 5, ANY, 96]),
    "sign": ("dgpu_sign", lambda c, a: calls.sign(c, C, 5, a.msgs, a.msg_len),
             lambda a: [C, ANY, a.n, P(a.msgs), 32, P(a.msg_len), ANY]),
    "make_partials_scheme": ("dgpu_make_partials_scheme",
                             lambda c, a: calls.make_partials_scheme(c, C, a.msgs, a.sidx, a.sidx, a.shares),
                             lambda a: [C, a.n, P(a.msgs), 2, P(a.sidx), P(a.sidx), P(a.shares), 4, ANY]),
    "verify_batch": ("dgpu_verify_batch", lambda c, a: calls.verify_batch(c, C, *recs(a), M, S),
                     lambda a: [C, *recs_args(a), M, S, ANY, ANY]),
    "verify_beacons": ("dgpu_verify_beacons", lambda c, a: calls.verify_beacons(c, C, PK, *recs(a), M, S),
                       lambda a: [C, ANY, 48, *recs_args(a), M, S, ANY, ANY]),
    "verify_multi": ("dgpu_verify_multi", lambda c, a: calls.verify_multi(c, C, PK, *recs(a), M, S),
                     lambda a: [C, ANY, 48, *recs_args(a), M, S, ANY, ANY]),
    "verify_recovered": ("dgpu_verify_recovered", lambda c, a: calls.verify_recovered(c, C, PK, *raw(a), M, S),
                         lambda a: [C, ANY, 48, a.n, *raw_args(a), M, S, ANY, ANY]),
    "verify_keyed": ("dgpu_verify_keyed", lambda c, a: calls.verify_keyed(c, C, a.keys, 48, a.idx, *raw(a), M, S),
                     lambda a: [C, 2, P(a.keys), 48, a.n, P(a.idx), *raw_args(a), M, S, ANY, ANY]),
    "verify_partials": ("dgpu_verify_partials", lambda c, a: calls.verify_partials(c, a.msgs, a.parts, a.plen, M, S),
                        lambda a: [*parts_args(a), M, S, ANY, ANY]),
    "recover_batch": ("dgpu_recover_batch",
                      lambda c, a: calls.recover_batch(c, a.msgs, a.parts, a.plen, 96, statuses=False),
                      lambda a: [*parts_args(a), ANY, ANY, None]),
    "recover_multi": ("dgpu_recover_multi",
                      lambda c, a: calls.recover_multi(c, a.msgs, a.parts, a.plen, 96, statuses=False),
                      lambda a: [*parts_args(a), ANY, ANY, None]),
    "verify_rows": ("dgpu_verify_rows", lambda c, a: calls.verify_rows(c, C, PK, a.base, a.off, a.ln, 96, 97, M, S),
                    lambda a: [C, ANY, 48, a.n, P(a.base), P(a.off), P(a.ln), 96, 97, M, S, ANY, ANY, ANY, ANY]),
    "verify_batch_device": ("dgpu_verify_batch_device",
                            lambda c, a: calls.verify_batch_device(c, C, *recs(a), M, S, a.bits, a.reason, STREAM),
                            lambda a: [C, *recs_args(a), M, S, P(a.bits), P(a.reason), STREAM]),
    "verify_beacons_device": ("dgpu_verify_beacons_device",
                              lambda c, a: calls.verify_beacons_device(c, C, PK, *recs(a), M, S, a.bits, None, STREAM),
                              lambda a: [C, ANY, 48, *recs_args(a), M, S, P(a.bits), None, STREAM]),
    "verify_keyed_device": ("dgpu_verify_keyed_device",
                            lambda c, a: calls.verify_keyed_device(c, C, a.keys, 48, a.idx, *raw(a), M, S, a.bits,
                                                                   a.reason, None),
                            lambda a: [C, 2, P(a.keys), 48, a.n, P(a.idx), *raw_args(a), M, S, P(a.bits), P(a.reason),
                                       None]),
    "verify_partials_device": ("dgpu_verify_partials_device",
                               lambda c, a: calls.verify_partials_device(c, a.msgs, a.parts, a.plen, M, S, a.bits,
                                                                         a.reason, STREAM),
                               lambda a: [*parts_args(a), M, S, P(a.bits), P(a.reason), STREAM]),
    "recover_batch_device": ("dgpu_recover_batch_device",
                             lambda c, a: calls.recover_batch_device(c, a.msgs, a.parts, a.plen, a.out, a.ok, None, STREAM),
                             lambda a: [*parts_args(a), P(a.out), P(a.ok), None, STREAM]),
    "decode_rows_device": ("dgpu_decode_rows_device",
                           lambda c, a: calls.decode_rows_device(c, a.base, a.off, a.ln, *recs(a), a.ok, STREAM),
                           lambda a: [a.n, P(a.base), a.base.size, P(a.off), P(a.ln), *recs_args(a)[1:], P(a.ok), STREAM]),
    "verify_segment_shard_device": ("dgpu_verify_segment_shard_device",
                                    lambda c, a: calls.verify_segment_shard_device(
                                        c, C, PK, 9, a.sigs, a.sig_len, a.halo, a.halo_len, M, S, a.bits, a.reason,
                                        None, STREAM),
                                    lambda a: [C, ANY, 48, *seg_args(a), P(a.halo), P(a.halo_len), M, S, P(a.bits),
                                               P(a.reason), None, STREAM]),
    "rlc_root_device": ("dgpu_rlc_root_device", lambda c, a: calls.rlc_root_device(c, C, PK, *recs(a), S, a.root, STREAM),
                        lambda a: [C, ANY, 48, *recs_args(a), S, P(a.root), STREAM]),
    "rlc_finish_device": ("dgpu_rlc_finish_device",
                          lambda c, a: calls.rlc_finish_device(c, 2, a.root, a.bits, None, STREAM),
                          lambda a: [2, P(a.root), P(a.bits), None, STREAM]),
    "synchronize": ("dgpu_synchronize", lambda c, a: calls.synchronize(c), lambda a: []),
    "multi_context": ("dgpu_multi_context", lambda c, a: calls.multi_context(c, 1), lambda a: [1, ANY]),
}
for _name in ("check_rows", "check_rows_multi"):
    CASES[_name] = ("dgpu_" + _name,
                    lambda c, a, f=getattr(calls, _name): f(c, C, PK, a.base, a.off, a.ln, a.rkeys, 96, 97, M, S, 10, 4),
                    lambda a: [C, ANY, 48, a.n, *rows_ptrs(a), 96, 97, M, S, 10, 4, ANY, ANY, 4, ANY,
                               ANY if a.n else None, a.n, ANY, None])
# the seed forms, with a seed and without one; a missing randomness output
for _seed, _tag, _sp in ((SEED, "", (ANY, 32)), (b"", "_no_seed", (None, 0))):
    for _name in ("verify_segment", "verify_segment_multi"):
        CASES[_name + _tag] = ("dgpu_" + _name,
                               lambda c, a, f=getattr(calls, _name), s=_seed: f(c, C, PK, 9, a.sigs, a.sig_len, s, M, S,
                                                                                randomness=not s),
                               lambda a, sp=_sp: [C, ANY, 48, *seg_args(a), *sp, M, S, ANY, ANY, None if sp[1] else ANY])
    CASES["verify_segment_device" + _tag] = (
        "dgpu_verify_segment_device",
        lambda c, a, s=_seed: calls.verify_segment_device(c, C, PK, 9, a.sigs, a.sig_len, s, M, S, a.bits, a.reason,
                                                          a.rand, STREAM),
        lambda a, sp=_sp: [C, ANY, 48, *seg_args(a), *sp, M, S, P(a.bits), P(a.reason), P(a.rand), STREAM])
    CASES["rlc_root_segment_device" + _tag] = (
        "dgpu_rlc_root_segment_device",
        lambda c, a, s=_seed: calls.rlc_root_segment_device(c, C, PK, 9, a.sigs, a.sig_len, s, None, None, S, a.root, STREAM),
        lambda a, sp=_sp: [C, ANY, 48, *seg_args(a), *sp, None, None, S, P(a.root), STREAM])


def same(got, want):
    if want is ANY:
        return got is not None
    if want is STREAM or (want is None and isinstance(got, ctypes.c_void_p)):
        return isinstance(got, ctypes.c_void_p) and got.value == (want.cuda_stream if want else None)
    return type(got) is type(want) and got == want


def test_cases_cover_the_module():
    """Every public function of the call module that reaches the library has
    a case (the helpers that make no call are listed)."""
    helpers = {"sig_width", "key_width", "rlc_seed_for", "pack_msgs", "check_bitmap", "profiled", "rlc_root_bytes", "ptr"}
    public = {k for k, v in vars(calls).items() if callable(v) and not k.startswith("_")} - helpers
    assert public == {k.replace("_no_seed", "").replace("_g1", "") for k in CASES}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_arguments(name, shape):
    symbol, call, expect = CASES[name]
    ctx, a = stub_ctx(), arrays(*SHAPES[shape])
    try:
        call(ctx, a)
    except _lib.DrandGPUError as e:  # the stub wrote no verdicts: a host verify form refuses them, after the call
        assert name.replace("_no_seed", "") in HOST_VERIFY and "disagree" in str(e)
    (got_symbol, got), = ctx.lib.seen
    want = [HANDLE] + expect(a)
    assert got_symbol == symbol and len(got) == ARGC[symbol] == len(want)
    assert got[0] is HANDLE
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got[1:], want[1:]), 1) if not same(g, w)]
    assert not bad, bad


def test_host_outputs_and_fill():
    """Host forms allocate outputs of the arrays' sizes, filled as asked; a
    fresh seed is drawn in RLC mode without one, none in per-round mode."""
    a = arrays(9, 96)
    # a library that writes nothing: zero reasons read "valid" under a zero bitmap, a sentinel fill does not
    with pytest.raises(_lib.DrandGPUError, match="disagree"):
        calls.verify_beacons(stub_ctx(), C, PK, a.rounds, a.sigs, a.sig_len, a.prev, a.prev_len)
    assert (calls.verify_beacons(stub_ctx(), C, PK, a.rounds, a.sigs, a.sig_len, a.prev, a.prev_len, fill=0xEE)
            == 0xEE).all()
    reason, rand = calls.verify_segment(stub_ctx(), C, PK, 1, a.sigs, a.sig_len, SEED, fill=0xEE)
    assert reason.shape == (9,) and rand.shape == (9, 32) and (reason == 0xEE).all() and (rand == 0xEE).all()
    out, ok, pv = calls.recover_batch(stub_ctx(), a.msgs, a.parts, a.plen, 48)
    assert out.shape == (9 * 48,) and ok.shape == (2,) and pv.shape == (18,)
    for mode, fresh in ((_lib.MODE_RLC, True), (_lib.MODE_PER_ROUND, False)):
        seeds = set()
        for _ in range(2):
            ctx = stub_ctx()
            calls.verify_segment(ctx, C, PK, 1, a.sigs, a.sig_len, SEED, mode, fill=0xEE)
            seeds.add(ctx.lib.seen[0][1][12])
        assert (len(seeds) == 2) == fresh and (fresh or seeds == {0})


def test_arrays_given_for_key_and_seed_are_passed_as_they_are():
    """A key or seed that is already a uint8 array is the caller's buffer: no copy."""
    a, pk, seed = arrays(3, 96), np.arange(48, dtype=np.uint8), np.full(32, 7, dtype=np.uint8)
    for s, want in ((seed, (P(seed), 32)), (np.zeros(0, dtype=np.uint8), (None, 0)), (None, (None, 0))):
        ctx = stub_ctx()
        calls.verify_segment_device(ctx, C, pk, 9, a.sigs, a.sig_len, s, M, S, a.bits, a.reason, a.rand)
        got = ctx.lib.seen[0][1]
        assert got[2:4] == (P(pk), 48) and got[9:11] == want


def test_profiled_and_root_bytes():
    ctx = stub_ctx()
    with calls.profiled(ctx) as stage_times:
        assert callable(stage_times)
    assert [(n, a[1]) for n, a in ctx.lib.seen] == [("dgpu_set_profiling", 1), ("dgpu_set_profiling", 0)]
    assert calls.rlc_root_bytes(ctx, C) == 576
    with pytest.raises(_lib.DrandGPUError, match="from stub"):
        calls.rlc_root_bytes(stub_ctx(rc=_lib.DGPU_EINVAL), C)


@pytest.mark.parametrize("name", CASES)
def test_error_is_the_contexts_library(name):
    """A failing call raises with the message of the context's own library,
    not the default build's."""
    _, call, _ = CASES[name]
    with pytest.raises(_lib.DrandGPUError, match="drand_gpu error -1: from stub") as e:
        call(stub_ctx(rc=-1), arrays(3, 96))
    assert e.value.code == -1


def test_set_group_records_the_group_on_the_context():
    ctx = stub_ctx()
    key = calls.set_group(ctx, C, 2, 5, [PK, PK])
    assert ctx.installed_group == key == (C, 5, (PK, PK))
    with pytest.raises(_lib.DrandGPUError):
        ctx.lib.rc = -1
        calls.set_group(ctx, C, 2, 5, [PK, PK])
    assert ctx.installed_group is None  # a failed install leaves no group on record


HOST_VERIFY = {
    "verify_batch": (12, 13), "verify_beacons": (14, 15), "verify_multi": (14, 15), "verify_segment": (13, 14),
    "verify_segment_multi": (13, 14), "verify_recovered": (13, 14), "verify_keyed": (15, 16), "verify_partials": (9, 10),
    "verify_rows": (14, 15),
}


@pytest.mark.parametrize("name", HOST_VERIFY)
def test_bitmap_and_reasons_must_agree(name):
    """The stub reports record 8 valid in the bitmap's second byte and invalid
    in the reasons; every host-form verify call refuses the result.  (With the
    bit cleared the same results pass.)"""
    bits_at, reason_at = HOST_VERIFY[name]
    n = 9 if name != "verify_partials" else 9 * 2

    def write(flip):
        def effect(_, args):
            bits = (ctypes.c_uint8 * ((n + 7) // 8)).from_address(args[bits_at])
            reason = (ctypes.c_uint8 * n).from_address(args[reason_at])
            for i in range(n):
                reason[i] = _lib.REASON_PAIRING
            bits[0], bits[(n - 1) // 8] = 0, (1 << ((n - 1) % 8)) if flip else 0
        return effect
    _, call, _ = CASES[name]
    call(stub_ctx(effect=write(False)), arrays(9, 96))
    with pytest.raises(_lib.DrandGPUError, match="disagree"):
        call(stub_ctx(effect=write(True)), arrays(9, 96))
