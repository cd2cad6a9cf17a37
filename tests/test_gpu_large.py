"""Parity at large N: GPU-generated chains of 1M
rounds (chained G2) and 1M rounds (bls-unchained-on-g1), 0.1% corrupted
across the whole catalog, verified on the GPU per round and in RLC mode (at
this size the bulk kernels run whatever DGPU_THR_MIN / DGPU_RLC_MIN say: the
per-thread T-steps and chains, the RLC root MSM).  Verdicts must equal the construction for every
round, RLC reasons must equal per-round reasons, and a stratified sample --
every corrupted round plus 1,500 uniformly drawn valid ones -- is re-verified
by the C restatement of the reference (oracle/c, test infrastructure) with
reasons compared one by one.  Marked gpu."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1_000_000
SAMPLE = 1500


def _sample(n, bad, seed):
    rng = np.random.default_rng(seed)
    valid = np.setdiff1d(np.arange(n), np.fromiter(bad.keys(), dtype=np.int64))
    return np.sort(np.concatenate([np.fromiter(bad.keys(), dtype=np.int64), rng.choice(valid, SAMPLE, replace=False)]))


def _reasons(code, c, mode):
    from drand_amd import calls
    from drand_amd.chain import get_context
    return calls.verify_beacons(get_context(0), code, c.pk, *c.records(), mode, 0xC0DE, fill=0xEE)


@pytest.mark.parametrize("code_name", ["SCHEME_CHAINED", "SCHEME_UNCHAINED_G1"])
def test_one_million_rounds_against_construction_and_c_oracle(code_name):
    from drand_amd import _lib
    from drand_amd.synth import corrupt, make_chain
    from oracle import c_ref
    code = getattr(_lib, code_name)
    c = make_chain(1234, N, code, seg_len=256)
    bad = corrupt(c, 1234, rate=1e-3)
    expect = np.ones(N, dtype=bool)
    expect[list(bad.keys())] = False
    per = _reasons(code, c, _lib.MODE_PER_ROUND)
    assert np.array_equal(per == 0, expect)
    rlc = _reasons(code, c, _lib.MODE_RLC)
    assert np.array_equal(rlc, per)
    idx = _sample(N, bad, 99)
    sub = [np.ascontiguousarray(a[idx]) for a in (c.rounds, c.sigs, c.sig_len, c.prev, c.prev_len)]
    threads = min(16, os.cpu_count() or 1)
    if code == _lib.SCHEME_CHAINED:
        ref = c_ref.verify_batch(True, c.pk, *sub, threads)
    else:
        ref = c_ref.verify_batch_g1(False, c.pk, sub[0], sub[1], sub[2], threads)
    # the C restatement tests G2 membership by [r]Q as kilic does; the GPU's
    # fused test reports the same class
    assert ref.tolist() == per[idx].tolist()
