"""dgpu_verify_keyed on the GPU: every record under its own key.

Keys come from dgpu_derive_pubkey over seeded secrets, signatures from
chain.sign, so a record is valid iff it was signed by the secret of the key it
names, over its message, and left intact: the expected verdicts are known by
construction.  The reasons are compared with dgpu_verify_recovered called once
per key (the contract in include/drand_gpu.h) and with the oracle-made fixture
tests/golden/keyed_identities.json.

The suite runs with DGPU_RLC_MIN=0 (conftest.py), so every DGPU_MODE_RLC call
below takes the per-key combination (keyed.cuh) whatever its size; its
verdicts and reasons must equal per-record mode's.
"""
import contextlib
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, open_ctx

sys.path.insert(0, ROOT)
from drand_amd import _lib, calls, chain, identity, synth  # noqa: E402
from drand_amd.scheme import get_scheme_by_id_with_default, list_schemes, scheme_code  # noqa: E402

pytestmark = pytest.mark.gpu

G2SIG = "pedersen-bls-chained"
G1SIG = "bls-unchained-g1-rfc9380"
BOTH = (G2SIG, G1SIG)
MODES = (_lib.MODE_PER_ROUND, _lib.MODE_RLC)
MSG_LENS = (0, 1, 32, 33, 200)
# the corruption kinds that apply to a raw message (CORRUPT_PREV alters a previous signature: none here)
KINDS = (synth.CORRUPT_X_BIT, synth.CORRUPT_Y_SIGN, synth.CORRUPT_OTHER_ROUND, synth.CORRUPT_INFINITY,
         synth.CORRUPT_TRUNCATED)


def _scheme(name):
    return get_scheme_by_id_with_default(name)


def _is_g1(name):
    return _scheme(name).sigs_on_g1


def _msg(i, length):
    out = b""
    k = 0
    while len(out) < length:
        out += (i * 1000003 + k).to_bytes(8, "big")
        k += 1
    return out[:length]


class Batch:
    """n records over a table of keys: record i names key idx[i] and is
    signed by that key's secret."""

    def __init__(self, name, n_keys, idx, seed=0):
        self.name, self.scheme = name, _scheme(name)
        self.code = scheme_code(self.scheme)
        ctx = chain.get_context(0)
        self.sks = [synth.derive_secret(7000 + seed * 1000 + j) for j in range(n_keys)]
        self.idx = list(idx)
        # a large table derives the keys in use only; an entry no record names repeats the first of them
        used = sorted(set(self.idx)) if n_keys > 64 else list(range(n_keys))
        derived = {j: calls.derive_pubkey(ctx, self.code, self.sks[j]) for j in used}
        self.keys = [derived.get(j, derived[used[0]]) for j in range(n_keys)]
        self.msgs = [_msg(i + 31 * seed, MSG_LENS[i % len(MSG_LENS)]) for i in range(len(self.idx))]
        self.sigs = [None] * len(self.idx)
        for j in sorted(set(self.idx)):
            mine = [i for i, k in enumerate(self.idx) if k == j]
            for i, s in zip(mine, chain.sign(self.sks[j], [self.msgs[i] for i in mine], self.scheme)):
                self.sigs[i] = s
        self.expect = [0] * len(self.idx)
        self.signed = list(self.sigs)

    def corrupt(self, i, kind):
        s = bytearray(self.sigs[i])
        if kind == synth.CORRUPT_X_BIT:
            s[47] ^= 1
            self.expect[i] = -1  # decode or subgroup: whichever the single-key path says
        elif kind == synth.CORRUPT_Y_SIGN:
            s[0] ^= 0x20
            self.expect[i] = _lib.REASON_PAIRING
        elif kind == synth.CORRUPT_OTHER_ROUND:
            j = next(k for k in range(len(self.idx)) if self.idx[k] == self.idx[i] and self.msgs[k] != self.msgs[i])
            s = bytearray(self.signed[j])
            self.expect[i] = _lib.REASON_PAIRING
        elif kind == synth.CORRUPT_INFINITY:
            s = bytearray(len(s))
            s[0] = 0xC0
            self.expect[i] = _lib.REASON_INFINITY
        elif kind == synth.CORRUPT_TRUNCATED:
            s = s[:len(s) // 2] if i & 1 else bytearray()
            self.expect[i] = _lib.REASON_DECODE
        self.sigs[i] = bytes(s)

    def run(self, mode=_lib.MODE_PER_ROUND, ctx=None, n=None, seed=12345):
        n = len(self.idx) if n is None else n
        return chain.verify_keyed(self.scheme, self.keys, self.idx[:n], self.msgs[:n], self.sigs[:n], mode, seed,
                                  ctx=ctx).tolist()

    def per_key(self, mode=_lib.MODE_PER_ROUND):
        """dgpu_verify_recovered once per key on that key's records."""
        out = [None] * len(self.idx)
        for j in sorted(set(self.idx)):
            mine = [i for i, k in enumerate(self.idx) if k == j]
            got = chain.verify_recovered(self.scheme, self.keys[j], [self.msgs[i] for i in mine],
                                         [self.sigs[i] for i in mine], mode, 777)
            for i, r in zip(mine, got):
                out[i] = int(r)
        return out

    def check_expect(self, got):
        for i, (g, e) in enumerate(zip(got, self.expect)):
            if e < 0:
                assert g in (_lib.REASON_DECODE, _lib.REASON_SUBGROUP), (i, g)
            else:
                assert g == e, (i, g, e)


@pytest.fixture(scope="module")
def mixed():
    """300 records over 5 keys (200 / 60 / 30 / 9 / 1) and a sixth key with no
    record, message lengths 0, 1, 32, 33, 200, every corruption kind."""
    out = {}
    for name in BOTH:
        idx = [0] * 200 + [1] * 60 + [2] * 30 + [3] * 9 + [4]
        rng = np.random.default_rng(5)
        rng.shuffle(idx)
        b = Batch(name, 6, idx)
        victims = [i for i in range(300) if idx[i] in (0, 1)][3::17][:2 * len(KINDS)]
        for v, kind in zip(victims, KINDS + KINDS):
            b.corrupt(v, kind)
        out[name] = b
    return out


# ---------------------------------------------------------------- golden parity
def _fixture_nodes(section):
    g = load_golden("keyed_identities.json")[section]
    good = [(bytes.fromhex(n["key"]), bytes.fromhex(n["sig"]), bytes.fromhex(n["hash"]), 0) for n in g["nodes"]]
    bad = [(bytes.fromhex(m["key"]), bytes.fromhex(m["sig"]), bytes.fromhex(m["hash"]), m["reason"])
           for m in g["mutations"]]
    # the mutated nodes between the good ones
    nodes = []
    for i, n in enumerate(good):
        nodes.append(n)
        if i < len(bad):
            nodes.append(bad[i])
    nodes += bad[len(good):]
    return g["scheme"], nodes


@pytest.mark.parametrize("section", ["identities", "g1_signatures"])
@pytest.mark.parametrize("mode", MODES)
def test_golden_reasons(section, mode):
    name, nodes = _fixture_nodes(section)
    got = chain.verify_keyed(_scheme(name), [n[0] for n in nodes], list(range(len(nodes))), [n[2] for n in nodes],
                             [n[1] for n in nodes], mode, 99).tolist()
    assert got == [n[3] for n in nodes]
    assert _lib.REASON_KEY in got and _lib.REASON_PAIRING in got


def test_unsigned_identities_returns_the_mutated_nodes():
    _, nodes = _fixture_nodes("identities")
    pairs = [(n[0], n[1]) for n in nodes]
    for n in nodes:
        assert identity.identity_hash(n[0]) == n[2]
    assert identity.unsigned_identities(pairs) == [(n[0], n[1]) for n in nodes if n[3] != 0]
    assert identity.valid_signature(*pairs[0]) and not identity.valid_signature(pairs[0][0], pairs[2][1])
    # a key of the wrong length is no key at all
    assert identity.identity_reasons([(b"\x01" * 47, pairs[0][1]), pairs[0]]) == [_lib.REASON_KEY, 0]


# ---------------------------------------------------------------- equals the single-key path
@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("mode", MODES)
def test_equals_verify_recovered_per_key(mixed, name, mode):
    b = mixed[name]
    got = b.run(mode)
    assert got == b.per_key(mode)
    b.check_expect(got)
    assert sum(1 for g in got if g) == 2 * len(KINDS)


@pytest.mark.parametrize("name", list_schemes())
def test_every_scheme_id(name):
    b = Batch(name, 3, [0, 1, 2, 1, 0, 2, 2], seed=3)
    b.corrupt(3, synth.CORRUPT_Y_SIGN)
    b.idx[5] = 0  # a valid signature under another key of the table
    b.expect[5] = _lib.REASON_PAIRING
    for mode in MODES:
        b.check_expect(b.run(mode))


def _device_call(ctx, b, idx, mode=_lib.MODE_PER_ROUND):
    """The device form over torch buffers on a non-default stream; nothing
    synchronises between the call and the read-back but the stream itself."""
    import torch
    kb, key_len, kidx, mb, ml, sb, sl = chain.pack_keyed(b.code, b.keys, [0] * len(idx), b.msgs, b.sigs)
    kidx = np.asarray(idx, dtype=np.uint32)
    n = len(idx)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev, non_blocking=True)
             for a in (kidx, mb, ml, sb, sl)]
        bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=dev)
        reason = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        calls.verify_keyed_device(ctx, b.code, kb, key_len, *t, mode, 5, bits, reason, stream)
        kb[:] = 0  # the table was copied before the call returned
        h_reason = reason.cpu()
        h_bits = bits.cpu()
    stream.synchronize()
    return calls.check_bitmap(h_bits.numpy(), h_reason.numpy()).tolist()


@pytest.mark.parametrize("name", BOTH)
def test_device_form_agrees_with_host_form(mixed, gpu_ctx, name):
    b = mixed[name]
    assert _device_call(gpu_ctx, b, b.idx) == b.run()


# ---------------------------------------------------------------- key failures
def _bad_keys(name):
    g = load_golden("keyed_identities.json")["g1_signatures" if _is_g1(name) else "identities"]
    return {m["kind"]: bytes.fromhex(m["key"]) for m in g["mutations"] if m["kind"].startswith("key_")}


@pytest.mark.parametrize("name", BOTH)
def test_rejected_keys_mark_exactly_their_records(gpu_ctx, name):
    bad = _bad_keys(name)
    assert sorted(bad) == ["key_identity", "key_off_curve", "key_outside_subgroup", "key_x_ge_p"]
    b = Batch(name, 2, [0, 1] * 8, seed=1)
    b.corrupt(0, synth.CORRUPT_Y_SIGN)
    # table: good 0, the four rejected keys, good 1
    table = [b.keys[0]] + [bad[k] for k in sorted(bad)] + [b.keys[1]]
    idx = [0 if k == 0 else 5 for k in b.idx]
    expect = list(b.expect)
    for j, i in enumerate((2, 3, 4, 5, 6, 7, 8, 9)):  # two records per rejected key
        idx[i] = 1 + j % 4
        expect[i] = _lib.REASON_KEY
    b.sigs[6] = b.sigs[6][:10]  # ... one of them with an undecodable signature: the key comes first
    b.keys, b.idx, b.expect = table, idx, expect
    for mode in MODES:
        assert b.run(mode) == expect
    assert _device_call(gpu_ctx, b, idx) == expect
    # an index outside the table: DGPU_EINVAL on the host, DGPU_REASON_KEY on the device
    out = list(idx)
    out[11] = len(table)
    with pytest.raises(ValueError):
        chain.pack_keyed(b.code, table, out, b.msgs, b.sigs)
    kb, key_len, _, mb, ml, sb, sl = chain.pack_keyed(b.code, table, idx, b.msgs, b.sigs)
    oi = np.asarray(out, dtype=np.uint32)
    bits, reason = np.zeros(2, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def host(n_keys, klen, n=16, null=False):
        p = (lambda a: None) if null else _lib.ptr
        return lib.dgpu_verify_keyed(h, b.code, n_keys, p(kb), klen, n, p(oi), p(mb), mb.shape[1], p(ml), p(sb),
                                     sb.shape[1], p(sl), 0, 0, p(bits), p(reason))
    assert host(len(table), key_len) == _lib.DGPU_EINVAL and b"key_idx[11]" in lib.dgpu_last_error()
    expect_dev = list(expect)
    expect_dev[11] = _lib.REASON_KEY
    assert _device_call(gpu_ctx, b, out) == expect_dev
    oi[11] = idx[11]
    assert host(len(table), key_len) == _lib.DGPU_OK and reason.tolist() == expect
    assert host(0, key_len) == _lib.DGPU_EINVAL
    assert host(65537, key_len) == _lib.DGPU_EINVAL
    assert host(len(table), 144 - key_len) == _lib.DGPU_EINVAL
    assert host(len(table), key_len, n=0, null=True) == _lib.DGPU_OK
    assert lib.dgpu_verify_keyed_device(h, b.code, 1, None, key_len, 0, None, None, 0, None, None, 0, None, 0, 0,
                                        None, None, None) == _lib.DGPU_OK
    assert host(len(table), key_len, n=16) == _lib.DGPU_OK
    bad_mode = lib.dgpu_verify_keyed(h, b.code, len(table), _lib.ptr(kb), key_len, 16, _lib.ptr(oi), _lib.ptr(mb),
                                     mb.shape[1], _lib.ptr(ml), _lib.ptr(sb), sb.shape[1], _lib.ptr(sl), 2, 0,
                                     _lib.ptr(bits), _lib.ptr(reason))
    assert bad_mode == _lib.DGPU_EINVAL
    ml[3] = mb.shape[1] + 1  # a message longer than its stride: an argument error of the host form
    assert host(len(table), key_len) == _lib.DGPU_EINVAL


# ---------------------------------------------------------------- sizes
@pytest.fixture(scope="module")
def pools():
    """257 records per table size K in {1, 2, 300}: record i names key 37 (i mod 24) mod K -- at K = 300, 24 keys
    spread over more than one 256-wide block of the table, most of its entries without a record."""
    return {(name, K): Batch(name, K, [(37 * (i % 24)) % K for i in range(257)], seed=2)
            for name in BOTH for K in (1, 2, 300)}


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("K", [1, 2, 300])
def test_sizes_and_table_sizes(pools, name, K):
    b = pools[(name, K)]
    for n in (1, 7, 64, 65, 257):
        v = n // 2
        saved = b.sigs[v]
        b.corrupt(v, synth.CORRUPT_Y_SIGN)
        try:
            for mode in MODES:
                b.check_expect(b.run(mode, n=n))
        finally:
            b.sigs[v], b.expect[v] = saved, 0


@pytest.mark.parametrize("name", BOTH)
def test_both_kernel_families(mixed, name):
    """Pairing batches under DGPU_THR_MIN items take the 12-lane lines kernel
    (k_eng_lines), the others the per-thread ones; both read per-item keys."""
    b = mixed[name]
    lanes = open_ctx({"DGPU_THR_MIN": "65536"})
    thread = open_ctx({"DGPU_THR_MIN": "0"})
    try:
        a, t = b.run(ctx=lanes), b.run(ctx=thread)
    finally:
        lanes.close()
        thread.close()
    assert a == t
    b.check_expect(a)


# ---------------------------------------------------------------- a larger batch, one dominant key
@pytest.fixture(scope="module")
def large():
    """n = 4,099: one group of 3,500, the other 599 records over 41 keys (one
    of them with a single record)."""
    out = {}
    for name in BOTH:
        idx = [0] * 3500 + [1 + i % 40 for i in range(598)] + [41]
        rng = np.random.default_rng(11)
        rng.shuffle(idx)
        out[name] = Batch(name, 42, idx, seed=4)
    return out


@pytest.fixture(scope="module")
def short_ranges():
    """The A/B build with 7 list entries per thread of the per-key sums: the
    group of 3,500 spans 500 ranges, and small groups share theirs."""
    ctx = open_ctx({"DGPU_KEYED_RANGE": "7"})
    yield ctx
    ctx.close()


def _profiled(ctx, fn):
    with calls.profiled(ctx) as stage_times:
        return fn(), stage_times()  # raises above DGPU_MAX_STAGES


@pytest.mark.parametrize("name", BOTH)
def test_large_batch_cases(large, gpu_ctx, short_ranges, name):
    b = large[name]
    idx = b.idx
    big = [i for i, k in enumerate(idx) if k == 0]
    single = idx.index(41)
    g7 = [i for i, k in enumerate(idx) if k == 7]
    g9 = [i for i, k in enumerate(idx) if k == 9]
    sigs0, msgs0, idx0 = list(b.sigs), list(b.msgs), list(b.idx)
    RLC_STAGES = {"keyed_keys", "keyed_gather", "keyed_leaves", "keyed_group", "keyed_sums", "keyed_prep"}

    def case(title, change, fallback):
        b.sigs, b.msgs, b.idx, b.expect = list(sigs0), list(msgs0), list(idx0), [0] * len(idx0)
        change()
        per_record, st0 = _profiled(gpu_ctx, lambda: b.run(_lib.MODE_PER_ROUND))
        b.check_expect(per_record)
        assert not ({"keyed_leaves", "keyed_sums", "keyed_fallback"} & set(st0)) and "keyed_gather" in st0, title
        for ctx in (gpu_ctx, short_ranges):
            got, st = _profiled(ctx, lambda: b.run(_lib.MODE_RLC, ctx=ctx))
            assert got == per_record, title
            assert RLC_STAGES <= set(st), (title, st)
            assert ("keyed_fallback" in st) == fallback, (title, st)
        return per_record

    assert case("clean", lambda: None, False) == [0] * 4099
    case("one bad record in the large group", lambda: b.corrupt(big[1234], synth.CORRUPT_Y_SIGN), True)
    case("one bad record in a singleton group", lambda: b.corrupt(single, synth.CORRUPT_Y_SIGN), True)
    case("every record of a group bad", lambda: [b.corrupt(i, synth.CORRUPT_Y_SIGN) for i in g7], True)
    # a group whose records all fail decode: no undecided record, no candidate, the statuses kept
    case("a group whose records all fail decode", lambda: [b.corrupt(i, synth.CORRUPT_TRUNCATED) for i in g9], False)

    def twice():
        b.sigs[big[5]], b.msgs[big[5]] = b.sigs[big[6]], b.msgs[big[6]]
    case("the same record twice in a group", twice, False)

    def swapped():  # each valid under the other's key
        i, j = g7[0], g9[0]
        b.idx[i], b.idx[j] = 9, 7
        b.expect[i] = b.expect[j] = _lib.REASON_PAIRING
    case("two records labelled with each other's key", swapped, True)


@pytest.mark.parametrize("name", BOTH)
def test_rlc_below_the_threshold_runs_per_record(mixed, name):
    """Under the library's default DGPU_RLC_MIN a small DGPU_MODE_RLC batch
    takes the per-record path."""
    b = mixed[name]
    with contextlib.closing(open_ctx({"DGPU_RLC_MIN": "131072"})) as ctx:
        got, st = _profiled(ctx, lambda: b.run(_lib.MODE_RLC, ctx=ctx))
    b.check_expect(got)
    assert "keyed_leaves" not in st and "keyed_gather" in st


# ---------------------------------------------------------------- cancelling errors inside one key's group
@pytest.mark.parametrize("name", BOTH)
def test_errors_that_cancel_in_a_plain_sum_are_caught(name):
    """sig_a + D and sig_b - D under one key, D another valid signature point:
    their plain sum is unchanged, so a per-key sum with coefficient 1 would
    pass.  Both must come out DGPU_REASON_PAIRING in RLC mode (the
    coefficients are applied), as they do per record."""
    from oracle import bls12381 as B
    b = Batch(name, 2, [0] * 6 + [1] * 3, seed=6)
    g1 = _is_g1(name)
    dec, comp, add, neg = ((B.g1_decompress, B.g1_compress, B.g1_add, B.g1_neg) if g1 else
                           (B.g2_decompress, B.g2_compress, B.g2_add, B.g2_neg))
    D = dec(b.sigs[5])
    b.sigs[1] = comp(add(dec(b.sigs[1]), D))
    b.sigs[2] = comp(add(dec(b.sigs[2]), neg(D)))
    b.expect[1] = b.expect[2] = _lib.REASON_PAIRING
    for mode in MODES:
        b.check_expect(b.run(mode))


# ---------------------------------------------------------------- staging and stages
@pytest.mark.parametrize("name", BOTH)
def test_staged_bytes_and_stage_count(mixed, gpu_ctx, name):
    b = mixed[name]
    _, _, _, mb, _, sb, _ = chain.pack_keyed(b.code, b.keys, b.idx, b.msgs, b.sigs)
    with calls.profiled(gpu_ctx) as stage_times:
        for mode in MODES:
            b.run(mode)
            assert _lib.staging_stats(gpu_ctx)[2] == 300 * (mb.shape[1] + sb.shape[1] + 12)
            stages = stage_times()  # raises above DGPU_MAX_STAGES
            assert {"keyed_keys", "keyed_gather", "eng_miller", "pack_verdicts"} <= set(stages)
