"""GPU parity of the two forms of fp_reduce_lz (fp.cuh) in the per-thread
lines and chain kernels: the reduction straight from lazy limbs (shipped) and
the carried form, which the A/B build keeps as k_kb_chain_thr<., false> and
k_lines_thr<., false> behind DGPU_REDUCE_NORM=1.

Every context has DGPU_THR_MIN=1, so the per-thread kernels run at every n.
The sizes cover one 5-round engine block and its boundary (5, 6), one wave
and its boundary (64, 65) and one 256-thread block and its boundary (257).
Marked gpu."""
import numpy as np
import pytest

from conftest import load_golden, open_ctx

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 6, 64, 65, 257]
# the shipped library, the A/B build in the shipped form, the A/B build in the carried form
ENVS = {"shipped": {"DGPU_THR_MIN": "1"},
        "ab_lazy": {"DGPU_THR_MIN": "1", "DGPU_REDUCE_NORM": "0"},
        "ab_norm": {"DGPU_THR_MIN": "1", "DGPU_REDUCE_NORM": "1"}}


@pytest.fixture(scope="module")
def ctxs():
    from drand_amd import _lib
    c = {k: open_ctx(e) for k, e in ENVS.items()}
    assert c["shipped"].lib is _lib.load() and c["ab_lazy"].lib is c["ab_norm"].lib is _lib.load(_lib.AB_LIB_PATH)
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
    """One seeded chained chain of 257 rounds; its prefixes are the cases."""
    from drand_amd import _lib
    from drand_amd.synth import make_chain
    return make_chain(15, max(SIZES), _lib.SCHEME_CHAINED, seg_len=64)


@pytest.mark.parametrize("mode", ["per_round", "rlc"])
@pytest.mark.parametrize("n", SIZES)
def test_synthetic_chain_forms_agree(ctxs, synthetic, n, mode):
    """The first n rounds with the corruption catalog applied: verdicts equal
    the construction, reasons equal between the forms and the builds."""
    from drand_amd import _lib
    from drand_amd.synth import Chain, corrupt
    s = synthetic
    c = Chain(s.scheme_code, s.pk, s.rounds[:n].copy(), s.sigs[:n].copy(), s.sig_len[:n].copy(), s.prev[:n].copy(),
              s.prev_len[:n].copy(), s.genesis)
    bad = corrupt(c, 15 + n, rate=2e-2)
    m = _lib.MODE_RLC if mode == "rlc" else _lib.MODE_PER_ROUND
    got = {k: _reasons(x, _lib.SCHEME_CHAINED, c.pk, c.rounds, c.sigs, c.sig_len, c.prev, c.prev_len, m)
           for k, x in ctxs.items()}
    assert got["shipped"] == got["ab_lazy"] == got["ab_norm"]
    assert [r == 0 for r in got["shipped"]] == [i not in bad for i in range(n)]


@pytest.mark.parametrize("mode", ["per_round", "rlc"])
@pytest.mark.parametrize("name", ["chain_chained_s1.json", "chain_on_g1_s1.json"])
def test_golden_chain_forms_agree(ctxs, name, mode):
    """The golden chains, valid rounds and corrupted ones: reasons equal the
    fixture's in both forms and builds."""
    from drand_amd import _lib
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    g = load_golden(name)
    code = scheme_code(get_scheme_by_id_with_default(g["scheme"]))
    recs = g["rounds"] + g["corrupted"]
    arrays = _pack([(bytes.fromhex(r.get("prev", "")), r["round"], bytes.fromhex(r["sig"])) for r in recs])
    expect = [0] * len(g["rounds"]) + [c["reason"] for c in g["corrupted"]]
    m = _lib.MODE_RLC if mode == "rlc" else _lib.MODE_PER_ROUND
    for k, x in ctxs.items():
        assert _reasons(x, code, bytes.fromhex(g["pk"]), *arrays, m) == expect, k


def test_recover_smallest_fixture_forms_agree(ctxs):
    """Threshold recovery of the t = 3 fixture: the recovered bytes and the
    failures equal the fixture's in both forms and builds."""
    from drand_amd.threshold import ThresholdGroup
    g = load_golden("recover_t3_n8.json")
    commits = [bytes.fromhex(c) for c in g["commits"]]
    msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
    parts = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
    for k, ctx in ctxs.items():
        sigs, valid = ThresholdGroup(commits, g["n"], ctx=ctx).recover_batch(msgs, parts)
        assert [s.hex() if s else None for s in sigs] == [c["recovered"] for c in g["cases"]], k
        assert [v for v in valid] == [c["valid"] for c in g["cases"]], k
