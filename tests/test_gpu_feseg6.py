"""GPU parity of the two kernels for the Karabina FE's segments 1..5:
k_eng_fe_seg6 (one Fp2 coefficient per lane, feseg6_kernels.cuh; the default)
against the 12-lane k_eng_fe_seg (DGPU_FESEG=lanes12).

Every context has DGPU_THR_MIN=1, so the six-lane kernel runs at every n;
each dispatch runs once plain and once with DGPU_KB_TEST_FLAG=3, which flags
every third item: those take their verdict from the fallback, and the
segments must leave them alone and list their blocks.  The sizes and
corruption maps are those of test_gpu_miller6.py (miller6_cases.py: one
5-round block, the 10-item wave and the 64-lane boundary, each with its
successor, valid rounds beside corrupted ones).  Marked gpu."""
import numpy as np
import pytest

from conftest import load_golden, open_ctx
from miller6_cases import CASES, CHAIN_SEED, RATE, SIZES, corrupt_seed, kinds_for

pytestmark = pytest.mark.gpu

ENVS = {"lanes6": {"DGPU_THR_MIN": "1"},
        "lanes12": {"DGPU_THR_MIN": "1", "DGPU_FESEG": "lanes12"},
        "lanes6_flag3": {"DGPU_THR_MIN": "1", "DGPU_KB_TEST_FLAG": "3"},
        "lanes12_flag3": {"DGPU_THR_MIN": "1", "DGPU_FESEG": "lanes12", "DGPU_KB_TEST_FLAG": "3"}}


@pytest.fixture(scope="module")
def ctxs():
    c = {k: open_ctx(e) for k, e in ENVS.items()}
    yield c
    for x in c.values():
        x.close()


def _reasons(ctx, scheme, pk, rounds, sigs, sig_len, prev, prev_len):
    from drand_amd import _lib, calls
    calls.set_pubkey(ctx, scheme, pk)
    return calls.verify_batch(ctx, scheme, rounds, sigs, sig_len, prev, prev_len, _lib.MODE_PER_ROUND, 7, fill=0xEE).tolist()


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


@pytest.mark.parametrize("n,corrupted", [(n, c) for n in SIZES for c in (False, True)])
def test_synthetic_chain_kernels_agree(ctxs, synthetic, n, corrupted):
    """The first n rounds, clean or corrupted as miller6_cases says: verdicts
    equal the construction, reasons equal between the kernels, flagged or not."""
    from drand_amd import _lib
    from drand_amd.synth import Chain, corrupt
    assert (n, True) in CASES
    s = synthetic
    c = Chain(s.scheme_code, s.pk, s.rounds[:n].copy(), s.sigs[:n].copy(), s.sig_len[:n].copy(), s.prev[:n].copy(),
              s.prev_len[:n].copy(), s.genesis)
    bad = corrupt(c, corrupt_seed(n), rate=RATE, kinds=kinds_for(n)) if corrupted else {}
    got = {k: _reasons(x, _lib.SCHEME_CHAINED, c.pk, c.rounds, c.sigs, c.sig_len, c.prev, c.prev_len)
           for k, x in ctxs.items()}
    for k in ENVS:
        assert got[k] == got["lanes12"], k
    assert [r == 0 for r in got["lanes6"]] == [i not in bad for i in range(n)]


@pytest.mark.parametrize("name", ["chain_chained_s1.json", "chain_on_g1_s1.json"])
def test_golden_chain_kernels_agree(ctxs, name):
    """A golden chain, valid rounds and corrupted ones, signatures on G2 and
    on G1: reasons equal the fixture's with both kernels, flagged or not."""
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    g = load_golden(name)
    code = scheme_code(get_scheme_by_id_with_default(g["scheme"]))
    recs = g["rounds"] + g["corrupted"]
    arrays = _pack([(bytes.fromhex(r.get("prev", "")), r["round"], bytes.fromhex(r["sig"])) for r in recs])
    expect = [0] * len(g["rounds"]) + [c["reason"] for c in g["corrupted"]]
    for k, x in ctxs.items():
        assert _reasons(x, code, bytes.fromhex(g["pk"]), *arrays) == expect, k


@pytest.mark.parametrize("n", [1, 11])
def test_contexts_run_the_kernels_they_name(synthetic, n):
    """Which FE segment kernel a call launches, from its stage marks: in the
    A/B build DGPU_TEST_FE_MARK=1 gives the six-lane launches a mark of their
    own.  The default dispatch runs k_eng_fe_seg6 (and verifies the rounds);
    DGPU_FESEG=lanes12 does not."""
    from drand_amd import _lib, calls
    s = synthetic
    seen = {}
    for k in ("lanes6", "lanes12"):
        ctx = open_ctx(dict(ENVS[k], DGPU_TEST_FE_MARK="1"))
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
    assert {"eng_fe", "eng_fe_seg6"} <= seen["lanes6"]
    assert "eng_fe" in seen["lanes12"] and "eng_fe_seg6" not in seen["lanes12"]
