"""GPU parity of the two Miller kernels: k_eng_miller6 with its norm tail (one
Fp2 coefficient per lane, miller6_kernels.cuh; the default) against the
12-lane k_eng_miller (DGPU_MILLER=lanes12).

Both contexts have DGPU_THR_MIN=1, so the six-lane kernel runs at every n.
The sizes cover one 5-round block, the 10-item wave and the 64-lane boundary,
each with its successor (miller6_cases.py, which also says how each size
keeps valid rounds beside corrupted ones).  Marked gpu."""
import numpy as np
import pytest

from conftest import load_golden, open_ctx
from miller6_cases import CASES, CHAIN_SEED, RATE, SIZES, corrupt_seed, kinds_for

pytestmark = pytest.mark.gpu

ENVS = {"lanes6": {"DGPU_THR_MIN": "1"},
        "lanes12": {"DGPU_THR_MIN": "1", "DGPU_MILLER": "lanes12"}}


@pytest.fixture(scope="module")
def ctxs():
    c = {k: open_ctx(e) for k, e in ENVS.items()}
    yield c
    for x in c.values():
        x.close()


def _reasons(ctx, scheme, pk, rounds, sigs, sig_len, prev, prev_len, mode):
    from drand_amd import calls
    calls.set_pubkey(ctx, scheme, pk)
    return calls.verify_batch(ctx, scheme, rounds, sigs, sig_len, prev, prev_len, mode, 7, fill=0xEE).tolist()


def _pack(beacons):
    n = len(beacons)
    rounds = np.array([b[1] for b in beacons], dtype=np.uint64)
    sigs, prev = np.zeros((n, 96), dtype=np.uint8), np.zeros((n, 96), dtype=np.uint8)
    sig_len, prev_len = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for i, (p, _, s) in enumerate(beacons):
        sigs[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        prev[i, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        sig_len[i], prev_len[i] = len(s), len(p)
    return rounds, sigs, sig_len, prev, prev_len


@pytest.fixture(scope="module")
def synthetic():
    """One seeded chained chain of 65 rounds; its prefixes are the cases."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    return make_chain(CHAIN_SEED, max(SIZES), _lib.SCHEME_CHAINED, seg_len=64)


@pytest.mark.parametrize("mode", ["per_round", "rlc"])
@pytest.mark.parametrize("n,corrupted", CASES)
def test_synthetic_chain_kernels_agree(ctxs, synthetic, n, corrupted, mode):
    """The first n rounds, corrupted as miller6_cases says: verdicts equal the
    construction, reasons equal between the two kernels."""
    from drand_amd import _lib
    from drand_amd.synth import Chain, corrupt
    s = synthetic
    c = Chain(s.scheme_code, s.pk, s.rounds[:n].copy(), s.sigs[:n].copy(), s.sig_len[:n].copy(), s.prev[:n].copy(),
              s.prev_len[:n].copy(), s.genesis)
    bad = corrupt(c, corrupt_seed(n), rate=RATE, kinds=kinds_for(n)) if corrupted else {}
    m = _lib.MODE_RLC if mode == "rlc" else _lib.MODE_PER_ROUND
    got = {k: _reasons(x, _lib.SCHEME_CHAINED, c.pk, c.rounds, c.sigs, c.sig_len, c.prev, c.prev_len, m)
           for k, x in ctxs.items()}
    assert got["lanes6"] == got["lanes12"]
    assert [r == 0 for r in got["lanes6"]] == [i not in bad for i in range(n)]


@pytest.mark.parametrize("mode", ["per_round", "rlc"])
def test_golden_chain_kernels_agree(ctxs, mode):
    """The golden chained chain, valid rounds and corrupted ones: reasons
    equal the fixture's with both kernels."""
    from drand_amd import _lib
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    g = load_golden("chain_chained_s1.json")
    code = scheme_code(get_scheme_by_id_with_default(g["scheme"]))
    recs = g["rounds"] + g["corrupted"]
    arrays = _pack([(bytes.fromhex(r.get("prev", "")), r["round"], bytes.fromhex(r["sig"])) for r in recs])
    expect = [0] * len(g["rounds"]) + [c["reason"] for c in g["corrupted"]]
    m = _lib.MODE_RLC if mode == "rlc" else _lib.MODE_PER_ROUND
    for k, x in ctxs.items():
        assert _reasons(x, code, bytes.fromhex(g["pk"]), *arrays, m) == expect, k


@pytest.mark.parametrize("n", [1, 11])
def test_contexts_run_the_kernels_they_name(synthetic, n):
    """Which Miller kernels a call launches, from its stage marks: in the A/B
    build DGPU_TEST_MILLER_MARK=1 gives the six-lane launches marks of their
    own.  The default dispatch runs k_eng_miller6 and the tail (and verifies
    the rounds); DGPU_MILLER=lanes12 runs neither."""
    from drand_amd import _lib, calls
    s = synthetic
    seen = {}
    for k, env in ENVS.items():
        ctx = open_ctx(dict(env, DGPU_TEST_MILLER_MARK="1"))
        try:
            assert ctx.lib is _lib.load(_lib.AB_LIB_PATH)
            calls.set_pubkey(ctx, _lib.SCHEME_CHAINED, s.pk)
            with calls.profiled(ctx) as stage_times:
                got = calls.verify_batch(ctx, _lib.SCHEME_CHAINED, s.rounds[:n], s.sigs[:n], s.sig_len[:n], s.prev[:n],
                                         s.prev_len[:n], _lib.MODE_PER_ROUND, 7, fill=0xEE).tolist()
                seen[k] = set(stage_times())
            assert got == [0] * n, k
        finally:
            ctx.close()
    assert {"eng_miller", "eng_miller6", "eng_miller_tail"} <= seen["lanes6"]
    assert "eng_miller" in seen["lanes12"] and not {"eng_miller6", "eng_miller_tail"} & seen["lanes12"]


def test_recover_smallest_fixture_kernels_agree(ctxs):
    """Threshold recovery of the t = 3 fixture: the recovered bytes and the
    failures equal the fixture's with both kernels."""
    from drand_amd.threshold import ThresholdGroup
    g = load_golden("recover_t3_n8.json")
    commits = [bytes.fromhex(c) for c in g["commits"]]
    msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
    parts = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
    for k, ctx in ctxs.items():
        sigs, valid = ThresholdGroup(commits, g["n"], ctx=ctx).recover_batch(msgs, parts)
        assert [s.hex() if s else None for s in sigs] == [c["recovered"] for c in g["cases"]], k
        assert [v for v in valid] == [c["valid"] for c in g["cases"]], k
