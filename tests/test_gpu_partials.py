"""dgpu_verify_partials on the GPU: VerifyPartial of every slot under the
installed group, without a recovery (chain/beacon/node.go:117-125).

The suite runs with DGPU_RLC_MIN=0 (conftest.py), so every DGPU_MODE_RLC call
below takes the per-key combination with the share index as the key
(keyed.cuh); test_constructed_batch asserts its stages are recorded."""
import contextlib

import numpy as np
import pytest

from conftest import load_golden
from drand_amd import _lib, calls, synth
from drand_amd.threshold import ThresholdGroup

pytestmark = pytest.mark.gpu

MODES = (_lib.MODE_PER_ROUND, _lib.MODE_RLC)
FIXTURES = [("recover_t3_n8.json", None), ("recover_t17_n32.json", None),
            ("recover_g1_on_g1_t3_n8.json", "bls-unchained-on-g1")]


RLC_STAGES = {"keyed_leaves", "keyed_group", "keyed_sums", "keyed_prep"}


def _profiled(grp, fn):
    with calls.profiled(grp.ctx) as stage_times:
        return fn(), stage_times()  # raises above DGPU_MAX_STAGES


@pytest.mark.parametrize("name,scheme", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_fixture_slot_verdicts(name, scheme, mode):
    g = load_golden(name)
    assert scheme is None or g["scheme"] == scheme
    grp = ThresholdGroup([bytes.fromhex(c) for c in g["commits"]], g["n"], scheme=scheme)
    msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
    parts = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
    reasons = grp.verify_partials(msgs, parts, mode)
    for c, r in zip(g["cases"], reasons):
        assert [x == _lib.REASON_OK for x in r] == c["valid"], c["kind"]


@pytest.mark.parametrize("scheme", [_lib.SCHEME_CHAINED, _lib.SCHEME_G1_RFC9380])
def test_constructed_batch(scheme):
    """64 rounds x 17 slots, a wrong index in about a quarter of the rounds,
    plus a slot whose index lies above the group's table (signed by that
    index's share: the key is evaluated on the fly), an empty slot and a slot
    one byte short."""
    t, n, nr = 17, 32, 64
    group = synth.make_group(41, t, n, scheme=scheme)
    msgs, parts, ok = synth.make_recovery_batch(group, nr, 9, bad_rate=0.25)
    assert 4 < int((~ok).sum()) < nr - 4
    plen = parts.shape[2]
    # which slot of a bad round carries the wrong label: its label is not its signer's index, which the
    # batch does not return; a slot is good iff it verifies under its label, so rebuild the labels' truth
    # from a second signing with the labels as signers
    labels = (parts[:, :, 0].astype(np.uint32) << 8) | parts[:, :, 1]
    honest = synth.sign_partials(group, msgs, labels)
    good = (parts == honest).all(axis=2)
    assert np.array_equal(good.all(axis=1), ok)
    lists = [[bytes(parts[r, j]) for j in range(t)] for r in range(nr)]
    expect = [[_lib.REASON_OK if good[r, j] else _lib.REASON_PAIRING for j in range(t)] for r in range(nr)]
    # index 40 >= n, signed by share f(41)
    far = 40
    group.shares.append(synth.poly_eval(group.coeffs, far + 1))
    one = synth.sign_partials(group, msgs[3:4], np.array([[len(group.shares) - 1]], dtype=np.uint32),
                              np.array([[far]], dtype=np.uint32))
    group.shares.pop()
    lists[3][2] = bytes(one[0, 0])
    expect[3][2] = _lib.REASON_OK
    lists[5][0] = b""
    expect[5][0] = _lib.REASON_DECODE
    lists[7][16] = lists[7][16][:plen - 1]  # 97 bytes under a G2-signature group
    expect[7][16] = _lib.REASON_DECODE
    grp = ThresholdGroup(group.commits, n, scheme=scheme)
    mlist = [bytes(m) for m in msgs]
    got, stages = {}, {}
    for mode in MODES:
        got[mode], stages[mode] = _profiled(grp, lambda: grp.verify_partials(mlist, lists, mode, 4242))
    assert got[_lib.MODE_PER_ROUND] == got[_lib.MODE_RLC] == expect
    # RLC mode (the suite runs with DGPU_RLC_MIN=0) takes the per-key combination with the share index as the
    # group; the wrong labels fail their groups and the index above the table goes to the exact check
    assert RLC_STAGES <= set(stages[_lib.MODE_RLC]) and "keyed_fallback" in stages[_lib.MODE_RLC]
    assert not ((RLC_STAGES | {"keyed_fallback"}) & set(stages[_lib.MODE_PER_ROUND]))
    # the rounds without a bad or special slot: every group passes, nothing is left to the exact check
    clean = [r for r in range(nr) if ok[r] and r not in (3, 5, 7)]
    res, st = _profiled(grp, lambda: grp.verify_partials([mlist[r] for r in clean], [lists[r] for r in clean],
                                                         _lib.MODE_RLC, 4243))
    assert res == [[0] * t for _ in clean]
    assert RLC_STAGES <= set(st) and "keyed_fallback" not in st
    # the recovery reports the same validity wherever it reports a slot at all (it stops after t good ones,
    # so a round's later slots may be unreported: False there)
    _, valid = grp.recover_batch(mlist, lists, statuses=True)
    for r in range(nr):
        for j in range(t):
            if valid[r][j]:
                assert expect[r][j] == _lib.REASON_OK, (r, j)
        if all(e == _lib.REASON_OK for e in expect[r]):
            assert all(valid[r]), r


@pytest.mark.parametrize("scheme", [_lib.SCHEME_CHAINED, _lib.SCHEME_G1_RFC9380])
def test_errors_that_cancel_inside_a_share_group_are_caught(scheme):
    """Two rounds' partials of one share index, sig_a + D and sig_b - D with D
    another valid signature point: the share's plain sum is unchanged, so a
    per-key sum with coefficient 1 would pass.  Both must fail the pairing in
    RLC mode (the coefficients are applied), as they do per record."""
    from oracle import bls12381 as B
    t, n, nr = 3, 8, 6
    group = synth.make_group(43, t, n, scheme=scheme)
    msgs = np.frombuffer(b"".join(bytes([r + 1]) * 32 for r in range(nr)), dtype=np.uint8).reshape(nr, 32).copy()
    idx = np.tile(np.array([1, 4, 6], dtype=np.uint32), (nr, 1))
    parts = synth.sign_partials(group, msgs, idx)
    lists = [[bytes(parts[r, j]) for j in range(t)] for r in range(nr)]
    g1 = scheme == _lib.SCHEME_G1_RFC9380
    dec, comp, add, neg = ((B.g1_decompress, B.g1_compress, B.g1_add, B.g1_neg) if g1 else
                           (B.g2_decompress, B.g2_compress, B.g2_add, B.g2_neg))
    D = dec(lists[5][2][2:])
    lists[0][1] = lists[0][1][:2] + comp(add(dec(lists[0][1][2:]), D))
    lists[2][1] = lists[2][1][:2] + comp(add(dec(lists[2][1][2:]), neg(D)))
    expect = [[0] * t for _ in range(nr)]
    expect[0][1] = expect[2][1] = _lib.REASON_PAIRING
    grp = ThresholdGroup(group.commits, n, scheme=scheme)
    mlist = [bytes(m) for m in msgs]
    for mode in MODES:
        assert grp.verify_partials(mlist, lists, mode, 77) == expect


def test_no_group_installed():
    with contextlib.closing(_lib.Context(0)) as ctx:
        msgs = np.zeros(32, dtype=np.uint8)
        parts = np.zeros(98, dtype=np.uint8)
        plen = np.full(1, 98, dtype=np.uint32)
        bits = np.zeros(1, dtype=np.uint8)
        rc = ctx.lib.dgpu_verify_partials(ctx.handle, 1, _lib.ptr(msgs), 1, _lib.ptr(parts), 98, _lib.ptr(plen), 0, 0,
                                          _lib.ptr(bits), None)
        assert rc == _lib.DGPU_ENOKEY
        assert ctx.lib.dgpu_verify_partials(ctx.handle, 0, None, 1, None, 98, None, 0, 0, None, None) == _lib.DGPU_OK
        assert ctx.lib.dgpu_verify_partials_device(ctx.handle, 1, _lib.ptr(msgs), 1, _lib.ptr(parts), 98,
                                                   _lib.ptr(plen), 0, 0, _lib.ptr(bits), None,
                                                   None) == _lib.DGPU_ENOKEY
