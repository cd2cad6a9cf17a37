"""k_h2c_finish's park region at the edges of its 64-round blocks.

The cofactor ladder parks its cold points in wave-blocked slots
(kernels.cuh h2c_finish_stash): a block is 64 consecutive rounds, the region
is sized by whole blocks, and the kernel launches 256-thread blocks.  A
chained chain is verified per round on the bulk path (the suite's settings,
tests/conftest.py, send small batches through k_h2c_finish) with n = 63, 64,
65, 127, 129, 255, 257 and 1025 rounds -- a block less one, a whole block, a
block and one, and the same around two park blocks, one launch block and four
launch blocks -- and verdicts and reasons must equal the C restatement's
(oracle.c_ref) round by round.

Every corruption kind of synth.corrupt is present in every batch.  Each n is
verified twice: with its last round valid, and with that round's y-sign
flipped as well.  So a valid and a corrupted round both land in the last
block, whether it holds many rounds (the second batch alone has both there)
or a single one (n = 65, 129, 257, 1025: one batch each way).

At n = 65 the A/B build's forced-exceptional hook (DGPU_TEST_FORCE_EXC=1)
flags every round, so k_h2c_finish_redo recomputes each with the generic
form from P, read back from slot 0 of the region through get(0): the
verdicts must be the same.  Marked gpu."""
import contextlib
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

SIZES = (63, 64, 65, 127, 129, 255, 257, 1025)
BLOCK = 64


@functools.lru_cache(maxsize=None)
def _case(n):
    """(chain with its last round valid, {index: kind}, C restatement's reasons) for n rounds."""
    from drand_amd import _lib
    from drand_amd.synth import ALL_CORRUPTIONS, corrupt, make_chain
    from oracle import c_ref
    c = make_chain(900 + n, n, _lib.SCHEME_CHAINED, seg_len=64)
    clean = [a.copy() for a in (c.sigs, c.sig_len, c.prev)]
    for seed in range(900 + n, 964 + n):  # a seeded pattern that leaves the last round valid
        c.sigs[:], c.sig_len[:], c.prev[:] = clean
        bad = corrupt(c, seed, rate=0.05)
        if n - 1 not in bad:
            break
    assert n - 1 not in bad
    assert set(bad.values()) == set(ALL_CORRUPTIONS)
    ref = c_ref.verify_batch(True, c.pk, c.rounds, c.sigs, c.sig_len, c.prev, c.prev_len, min(16, os.cpu_count() or 1))
    return c, bad, ref


def _reasons(ctx, c):
    from drand_amd import _lib, calls
    return calls.verify_beacons(ctx, _lib.SCHEME_CHAINED, c.pk, *c.records(), fill=0xEE)


def _check_both_ways(ctx, n):
    """Reasons equal the C restatement's with the last round valid, then with its y-sign flipped."""
    from oracle import c_ref
    c, bad, ref = _case(n)
    last_block = range((n - 1) // BLOCK * BLOCK, n)
    got = _reasons(ctx, c)
    assert got.tolist() == ref.tolist()
    assert ref[n - 1] == 0 and all((ref[i] != 0) for i in bad)
    c.sigs[n - 1, 0] ^= 0x20
    try:
        ref2 = ref.copy()
        ref2[n - 1] = c_ref.verify_beacon(True, c.pk, int(c.rounds[n - 1]), bytes(c.prev[n - 1, :c.prev_len[n - 1]]),
                                          bytes(c.sigs[n - 1, :c.sig_len[n - 1]]))
        assert ref2[n - 1] != 0
        if len(last_block) > 1:  # a valid and a corrupted round in the last block of this one batch
            assert any(ref2[i] == 0 for i in last_block)
        got2 = _reasons(ctx, c)
    finally:
        c.sigs[n - 1, 0] ^= 0x20
    assert got2.tolist() == ref2.tolist()


@pytest.mark.parametrize("n", SIZES)
def test_park_block_edges_equal_c_restatement(gpu_ctx, n):
    assert os.environ.get("DGPU_COF_ENGINE_MAX") == "0"  # the suite's setting: small batches run k_h2c_finish
    _check_both_ways(gpu_ctx, n)


def test_generic_redo_reads_slot_0_of_the_park_region():
    from conftest import open_ctx
    n = 65
    with contextlib.closing(open_ctx({"DGPU_TEST_FORCE_EXC": "1"})) as ctx:
        _check_both_ways(ctx, n)
