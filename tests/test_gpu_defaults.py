"""The shipped kernel-selection thresholds: tests/conftest.py
sets DGPU_THR_MIN=0, DGPU_RLC_MIN=0, DGPU_COF_ENGINE_MAX=0 and DGPU_FE_GS_MAX=0
for the suite so that its small batches run the per-thread kernels, the RLC
pipeline, k_h2c_finish and the Karabina FE the bulk path uses.
These tests open fresh contexts at the library's defaults instead
(DGPU_THR_MIN=65536: pairing chunks under 64Ki items on the 12-lane lines and
8-lane chain; DGPU_RLC_MIN=131072: smaller RLC-mode calls on the per-round
path; DGPU_COF_ENGINE_MAX=16384 / DGPU_FE_GS_MAX=16384: small calls clear the
hash cofactor on the engine ladder and take the Granger-Scott FE) for the pipelines the chained-G2 default tests in test_gpu_parity.py
do not cover: G1 signatures per round and in RLC mode (a call above the RLC
threshold, so the combination runs with its node checks on the lane
kernels), and threshold recovery.  Verdicts equal the construction / golden
fixtures.  Marked gpu.

Tests elsewhere that pin the defaults: test_gpu_parity.py
test_small_batches_on_lane_kernels, test_rlc_small_batches_take_per_round_path,
test_rlc_node_checks_on_either_kernel_family."""
import contextlib

import numpy as np
import pytest

from conftest import load_golden, open_ctx
from segment_helpers import DEFAULTS

pytestmark = pytest.mark.gpu



@contextlib.contextmanager
def _default_ctx(extra=None):
    ctx = open_ctx(dict(DEFAULTS, **(extra or {})))
    try:
        yield ctx
    finally:
        ctx.close()


def _verify(ctx, code, c, mode, seed=777):
    from drand_amd import calls
    return calls.verify_beacons(ctx, code, c.pk, *c.records(), mode, seed, fill=0xEE)


@pytest.mark.parametrize("code_name", ["SCHEME_UNCHAINED_G1", "SCHEME_G1_RFC9380"])
def test_g1_per_round_and_small_rlc_at_defaults(code_name):
    """5,003-round G1 chains, 1% corrupted: per-round mode (lane kernels under
    64Ki) and RLC mode under 128Ki rounds (the per-round path) give the same
    reasons, equal to the construction."""
    from drand_amd import _lib
    from drand_amd.synth import corrupt, make_chain
    code = getattr(_lib, code_name)
    c = make_chain(91, 5003, code, seg_len=64)
    bad = corrupt(c, 91, rate=1e-2)
    expect = np.ones(len(c), dtype=bool)
    expect[list(bad.keys())] = False
    with _default_ctx() as ctx:
        per = _verify(ctx, code, c, _lib.MODE_PER_ROUND)
        rlc = _verify(ctx, code, c, _lib.MODE_RLC)
    assert np.array_equal(per == 0, expect)
    assert rlc.tolist() == per.tolist()


def test_g1_rlc_above_threshold_at_defaults():
    """A 140,000-round bls-unchained-on-g1 chain (above DGPU_RLC_MIN) in RLC
    mode at the defaults: bucket-MSM root, plain-sum localization with node
    checks under 64Ki items on the lane kernels, confirmation -- verdicts
    equal the construction and per-round mode."""
    from drand_amd import _lib
    from drand_amd.synth import corrupt, make_chain
    code = _lib.SCHEME_UNCHAINED_G1
    c = make_chain(93, 140000, code, seg_len=64)
    bad = corrupt(c, 93, rate=2e-4)
    expect = np.ones(len(c), dtype=bool)
    expect[list(bad.keys())] = False
    with _default_ctx() as ctx:
        rlc = _verify(ctx, code, c, _lib.MODE_RLC)
        per = _verify(ctx, code, c, _lib.MODE_PER_ROUND)
    assert np.array_equal(rlc == 0, expect)
    assert rlc.tolist() == per.tolist()


@pytest.mark.parametrize("name", ["recover_t3_n8.json", "recover_t17_n32.json"])
def test_recover_at_defaults(name):
    """Threshold recovery on a context at the shipped thresholds (its
    VerifyPartial / VerifyRecovered pairings are small batches, so they run on
    the lane kernels): recovered signatures and per-partial statuses equal the
    golden fixtures."""
    from drand_amd.threshold import ThresholdGroup
    g = load_golden(name)
    msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
    partials = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
    with _default_ctx() as ctx:
        sigs, valid = ThresholdGroup([bytes.fromhex(x) for x in g["commits"]], g["n"], ctx=ctx).recover_batch(msgs, partials)
    for c, s, v in zip(g["cases"], sigs, valid):
        assert v == c["valid"], c["kind"]
        assert (s.hex() if s else None) == c["recovered"], c["kind"]


@pytest.mark.parametrize("rows", ["0", "1"])
def test_recover_batched_check_table_layouts(rows):
    """The batched recovery check (no per-partial statuses requested) with its
    window tables gathered from SoA planes or from 224-byte rows
    (DGPU_RECOVER_ROWS): recovered signatures equal the t=17-of-32 and
    t=12-of-20 fixtures case by case."""
    from drand_amd.threshold import ThresholdGroup
    for name in ("recover_t17_n32.json", "recover_t12_n20.json"):
        g = load_golden(name)
        msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
        partials = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
        # the SoA layout is an A/B variant: only the A/B build reads the knob
        with _default_ctx({"DGPU_RECOVER_ROWS": rows} if rows == "0" else None) as ctx:
            grp = ThresholdGroup([bytes.fromhex(x) for x in g["commits"]], g["n"], ctx=ctx)
            sigs, _ = grp.recover_batch(msgs, partials, statuses=False)
        assert [s.hex() if s else None for s in sigs] == [c["recovered"] for c in g["cases"]], name


@pytest.mark.parametrize("cof_max,fe_max", [("0", "0"), ("16384", "0"), ("0", "16384"), ("16384", "16384")])
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_small_calls_latency_paths(cof_max, fe_max, n):
    """The small-call latency paths, each on and off: per-round calls up to
    DGPU_COF_ENGINE_MAX rounds clear the hash's cofactor on the 12-lane
    ladder (pairing_engine.cuh k_cof_*) instead of k_h2c_finish, and pairing
    calls up to DGPU_FE_GS_MAX items take the Granger-Scott FE instead of the
    Karabina side.  A chained chain with 1% corrupted rounds gives the
    construction's verdicts in every combination."""
    from drand_amd import _lib
    from drand_amd.synth import corrupt, make_chain
    c = make_chain(97 + n, n, _lib.SCHEME_CHAINED, seg_len=min(64, n))
    bad = corrupt(c, 97, rate=1e-2) if n > 50 else {}
    expect = np.ones(n, dtype=bool)
    expect[list(bad.keys())] = False
    with _default_ctx({"DGPU_COF_ENGINE_MAX": cof_max, "DGPU_FE_GS_MAX": fe_max}) as ctx:
        per = _verify(ctx, _lib.SCHEME_CHAINED, c, _lib.MODE_PER_ROUND)
    assert np.array_equal(per == 0, expect)


@pytest.fixture(scope="module")
def default_and_suite_ctx():
    with _default_ctx() as dflt:
        suite = open_ctx({})  # the suite's settings (conftest.py): k_h2c_finish and the Karabina FE
        try:
            yield dflt, suite
        finally:
            suite.close()


@pytest.mark.parametrize("n", [1, 6, 64, 65])
def test_cofactor_engine_scratch_around_blocks(default_and_suite_ctx, n):
    """Small per-round calls at the shipped thresholds clear the hash's cofactor
    on the engine ladder, whose scratch (cof_tmp's planes and the ladder's line
    buffer) is sized by the call: n around the 5-round engine block and the
    64-round wave.  Items cycled from the chained fixture, valid and corrupted
    alike: verdicts and reasons equal the fixture's and those of a context at
    the suite's settings (k_h2c_finish)."""
    from drand_amd import _lib
    from drand_amd.chain import Beacon, pack_beacons
    from drand_amd.synth import Chain
    g = load_golden("chain_chained_s1.json")
    items = [(r["prev"], r["round"], r["sig"], 0) for r in g["rounds"]]
    items += [(c["prev"], c["round"], c["sig"], c["reason"]) for c in g["corrupted"]]
    pick = [items[(n + i) % len(items)] for i in range(n)]
    rounds, sigs, sig_len, prev, prev_len = pack_beacons([Beacon(bytes.fromhex(p), r, bytes.fromhex(s))
                                                          for p, r, s, _ in pick])
    c = Chain(_lib.SCHEME_CHAINED, bytes.fromhex(g["pk"]), rounds, sigs, sig_len, prev, prev_len, None)
    dflt, suite = default_and_suite_ctx
    got = _verify(dflt, _lib.SCHEME_CHAINED, c, _lib.MODE_PER_ROUND)
    ref = _verify(suite, _lib.SCHEME_CHAINED, c, _lib.MODE_PER_ROUND)
    assert got.tolist() == [it[3] for it in pick]
    assert got.tolist() == ref.tolist()
