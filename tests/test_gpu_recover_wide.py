"""Threshold groups above t = 32 on the GPU (dgpu_set_group_wide and the wide
recovery path, drand_amd/csrc/recover_wide.cuh).

drand's key.MinimumT(n) is n/2 + 1, so every group of 64 nodes and more has a
threshold above the narrow kernels' 32.  Shapes: (33, 65) the first wide t;
(65, 129) one more candidate than a 64-lane wave; (129, 200) an odd count over
several lane groups with n not a power of two.  Both signature groups.

Expected values come from construction: the interpolant is unique, so a
recovered signature is sk * H(msg) bit for bit (synth.group_signatures), and a
partial is valid iff it is whole and its label is its signer's index.  Which
rounds recover follows the reference's walk (kyber tbls.Recover): the first t
valid partials in input order, duplicates counted, then at least t distinct
indices.  At (33, 65) on G2 the walk batch is also compared with the oracle's
restatements on the same input: oracle.c_ref.recover (real pairings) on every
round, and the pure-Python oracle.drand_ref.recover on the three failing
rounds and one recovering round (33 G2 scalar multiplications: about 7 s per
recovering round, so one)."""
import contextlib
import copy
import functools
import hashlib

import numpy as np
import pytest

from conftest import open_ctx

pytestmark = pytest.mark.gpu

SHAPES = [(33, 65), (65, 129), (129, 200)]
SCHEME_NAMES = ["pedersen-bls-unchained", "bls-unchained-g1-rfc9380"]


def _code(name):
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    return scheme_code(get_scheme_by_id_with_default(name))


@functools.lru_cache(maxsize=None)
def _group(t, n, name):
    from drand_amd import synth
    return synth.make_group(4000 + t, t, n, scheme=_code(name))


def _msgs(nr, tag=b"wide"):
    return np.stack([np.frombuffer(hashlib.sha256(tag + bytes([r])).digest(), dtype=np.uint8) for r in range(nr)])


def _tg(g, **kw):
    from drand_amd.threshold import ThresholdGroup
    return ThresholdGroup(g.commits, g.n, scheme=g.scheme_code, **kw)


@functools.lru_cache(maxsize=None)
def _clean(t, n, name, nr=6):
    """nr rounds of exactly t valid partials from distinct random signers:
    (msgs, partial lists, expected signatures)."""
    from drand_amd import synth
    g = _group(t, n, name)
    rng = np.random.default_rng(t)
    msgs = _msgs(nr)
    idx = np.argsort(rng.random((nr, n)), axis=1)[:, :t].astype(np.uint32)
    parts = synth.sign_partials(g, msgs, idx)
    want = [bytes(s) for s in synth.group_signatures(g, msgs)]
    return [bytes(m) for m in msgs], [[bytes(p) for p in row] for row in parts], want


def _reference_walk(t, slots):
    """slots: (index or None, valid) per partial in input order.  True iff the
    reference recovers: stop after t valid ones, then t distinct indices."""
    good = [i for i, ok in slots if ok][:t]
    return len(good) == t and len(set(good)) >= t


@functools.lru_cache(maxsize=None)
def _walk_batch(t, n, name):
    """One batch with the reference's walk cases; returns (msgs, partial
    lists, expected valid flags, expected signatures or None)."""
    from drand_amd import synth
    g = _group(t, n, name)
    far = 300  # a share index >= n: its key is evaluated on the fly
    assert far >= n
    g2 = copy.copy(g)
    g2.shares = g.shares + [synth.poly_eval(g.coeffs, far + 1)]
    rng = np.random.default_rng(100 + t)
    order = [list(map(int, rng.permutation(n)[:t + 2])) for _ in range(7)]
    # per round: (signer position in the share array, label) per slot, then the edits
    rows = []
    o = order[0]  # t - 1 good and one invalid: failure
    rows.append([(s, s) for s in o[:t - 1]] + [(o[t - 1], (o[t - 1] + 1) % n)])
    o = order[1]  # an invalid one among the first t, a good one after it: recovers (exact path)
    rows.append([(s, s) for s in o[:3]] + [(o[3], (o[3] + 1) % n)] + [(s, s) for s in o[4:t + 1]])
    o = order[2]  # an index twice among the first t and a spare after it: the walk stops at t good, t - 1 distinct
    rows.append([(s, s) for s in o[:5]] + [(o[2], o[2])] + [(s, s) for s in o[5:t]])
    o = order[3]  # an index twice and nothing left
    rows.append([(s, s) for s in o[:5]] + [(o[2], o[2])] + [(s, s) for s in o[5:t - 1]])
    o = order[4]  # an empty slot and a truncated partial in the middle (edited below), t good ones in all
    rows.append([(s, s) for s in o[:t + 2]])
    o = order[5]  # a signer with index >= n among t good ones
    rows.append([(s, s) for s in o[:t - 1]] + [(n, far)])
    o = order[6]  # t good ones: the batched check decides it
    rows.append([(s, s) for s in o[:t]])
    assert len(rows[2]) == t + 1 and len(rows[3]) == t
    nr, m = len(rows), t + 2
    sidx = np.zeros((nr, m), dtype=np.uint32)
    lab = np.zeros((nr, m), dtype=np.uint32)
    for r, row in enumerate(rows):
        for j, (s, l) in enumerate(row):
            sidx[r, j], lab[r, j] = s, l
    msgs = _msgs(nr, b"walk")
    signed = synth.sign_partials(g2, msgs, sidx, lab)
    lists, valid, slots = [], [], []
    for r, row in enumerate(rows):
        ps = [bytes(signed[r, j]) for j in range(len(row))]
        ok = [(far if s == n else s) == l for s, l in row]
        if r == 4:
            ps[7], ok[7] = b"", False
            ps[9], ok[9] = ps[9][:40], False
        lists.append(ps)
        valid.append(ok)
        slots.append([(l if len(p) >= 2 else None, v) for (s, l), p, v in zip(row, ps, ok)])
    sigs = synth.group_signatures(g, msgs)
    want = [bytes(sigs[r]) if _reference_walk(t, slots[r]) else None for r in range(nr)]
    assert [w is not None for w in want] == [False, True, False, False, True, True, True]
    return [bytes(x) for x in msgs], lists, valid, want


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_group_installs_and_recovers(name):
    """ThresholdGroup of t = 33 commitments installs and recovers (the narrow
    entry points return DGPU_EINVAL for it); above DGPU_MAX_THRESHOLD the
    library's error is raised."""
    from drand_amd import _lib
    from drand_amd.threshold import ThresholdGroup
    g = _group(33, 65, name)
    msgs, parts, want = _clean(33, 65, name)
    grp = _tg(g)
    assert grp.t == 33
    sigs, valid = grp.recover_batch(msgs[:2], parts[:2])
    assert sigs == want[:2] and valid == [[True] * 33] * 2
    with pytest.raises(_lib.DrandGPUError) as e:
        ThresholdGroup([g.commits[0]] * (_lib.MAX_THRESHOLD + 1), 4096, scheme=g.scheme_code)
    assert e.value.code == _lib.DGPU_EINVAL
    assert grp.recover(msgs[2], parts[2]) == want[2]  # the rejected call left the group installed


@pytest.mark.parametrize("name", SCHEME_NAMES)
@pytest.mark.parametrize("t,n", SHAPES)
@pytest.mark.parametrize("statuses", [True, False])
def test_gpu_wide_clean_rounds(t, n, name, statuses):
    """Exactly t valid partials from distinct random signers recover the group
    signature, with and without per-partial statuses.  Both go through the
    batched check (nothing decodable is left beyond the t candidates, so the
    statuses need no pairing of their own); the exact per-partial path is the
    walk batch's."""
    msgs, parts, want = _clean(t, n, name)
    sigs, valid = _tg(_group(t, n, name)).recover_batch(msgs, parts, statuses=statuses)
    assert sigs == want
    assert valid == ([[True] * t] * len(msgs) if statuses else None)


@pytest.mark.parametrize("name", SCHEME_NAMES)
@pytest.mark.parametrize("t,n", SHAPES)
def test_gpu_wide_reference_walk(t, n, name):
    msgs, lists, valid, want = _walk_batch(t, n, name)
    grp = _tg(_group(t, n, name))
    sigs, got_valid = grp.recover_batch(msgs, lists, statuses=True)
    assert got_valid == valid
    assert sigs == want
    sigs, none = grp.recover_batch(msgs, lists, statuses=False)
    assert none is None and sigs == want


def test_gpu_wide_reference_walk_matches_the_oracles():
    """(33, 65), G2 signatures: the same walk batch through the oracle's C
    restatement (every round, real pairings) and its Python restatement (the
    failing rounds and the exact-path round, verdicts by construction)."""
    from oracle import c_ref
    from oracle import drand_ref as D
    t, n = 33, 65
    g = _group(t, n, SCHEME_NAMES[0])
    msgs, lists, valid, want = _walk_batch(t, n, SCHEME_NAMES[0])
    sigs, _ = _tg(g).recover_batch(msgs, lists, statuses=False)
    assert sigs == want
    for r in range(len(msgs)):
        assert c_ref.recover(g.commits, t, msgs[r], lists[r]) == sigs[r], r
    # t - 1 good and one invalid: failure; an invalid one among the first t: recovered; the two duplicate rounds,
    # where the restatement's sort-and-dedupe is not c_ref's walk (both fail before any scalar multiplication)
    for r in (0, 1, 2, 3):
        known = {p: v for p, v in zip(lists[r], valid[r])}
        verdict = lambda i, s, k=known: k.get(i.to_bytes(2, "big") + s, False)  # noqa: E731
        assert D.recover(None, msgs[r], lists[r], t, n, verify=verdict) == sigs[r], r


def test_gpu_wide_cancelling_partials_rejected():
    """tests/test_recover.py::_cancelling_partials at t = 33: sig_0 + l_1 D and
    sig_1 - l_0 D leave sum_j l_j sig_j the group signature, yet both fail
    VerifyPartial; the batched check's random coefficients expose them."""
    from drand_amd import synth
    from oracle import bls12381 as B
    from oracle import drand_ref as D
    t, n = 33, 65
    g = _group(t, n, SCHEME_NAMES[0])
    msgs = _msgs(1, b"cancel")
    idx = np.array([list(range(3, 3 + t + 2))], dtype=np.uint32)
    parts = [bytes(p) for p in synth.sign_partials(g, msgs, idx)[0]]
    lam = D.lagrange_at_zero([int(i) + 1 for i in idx[0, :t]])
    Dp = B.g2_mul(B.G2_GEN, 0x1234567)
    s0 = B.g2_add(B.g2_decompress(parts[0][2:]), B.g2_mul(Dp, lam[1]))
    s1 = B.g2_add(B.g2_decompress(parts[1][2:]), B.g2_neg(B.g2_mul(Dp, lam[0])))
    parts[0] = parts[0][:2] + B.g2_compress(s0)
    parts[1] = parts[1][:2] + B.g2_compress(s1)
    sig = bytes(synth.group_signatures(g, msgs)[0])
    msg = bytes(msgs[0])
    grp = _tg(g)
    for _ in range(2):  # fresh coefficients per call
        got, _ = grp.recover_batch([msg, msg], [parts[:t], parts], statuses=False)
        assert got == [None, sig]
    got, valid = grp.recover_batch([msg, msg], [parts[:t], parts], statuses=True)
    assert got == [None, sig]
    assert valid == [[False, False] + [True] * (t - 2), [False, False] + [True] * t]


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_verify_partials_modes_agree(name):
    """dgpu_verify_partials under a wide group: per-record and RLC mode give
    the same reasons on a batch with one bad partial for each of two shares
    (and an index >= n, whose key is evaluated on the fly)."""
    from drand_amd import _lib
    msgs, lists, valid, _ = _walk_batch(33, 65, name)
    grp = _tg(_group(33, 65, name))
    rows = [0, 1, 5, 6]  # bad partials under two different labels, the index >= n, a clean round
    m = [msgs[r] for r in rows]
    p = [lists[r] for r in rows]
    per = grp.verify_partials(m, p, _lib.MODE_PER_ROUND)
    rlc = grp.verify_partials(m, p, _lib.MODE_RLC, 4242)
    assert per == rlc
    assert [[x == _lib.REASON_OK for x in row] for row in per] == [valid[r] for r in rows]
    assert sum(x == _lib.REASON_PAIRING for row in per for x in row) == 2


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_chunked_tables_equal_unchunked(name):
    """The A/B build's DGPU_RECOVER_WIDE_BUDGET sets the window tables' byte
    budget to three rounds of t = 33: 7 rounds take three chunks (3 + 3 + 1)
    and give the unchunked call's output byte for byte.  Under a lowered
    budget that build marks every chunk as a stage of a profiled call: the
    first pass over the 7 rounds shows chunks 0, 1, 2 and no fourth (the exact
    path's 3 rounds are one more chunk 0), the unlowered call shows none."""
    from drand_amd import _lib, calls
    from drand_amd.threshold import pack_partials
    t, n = 33, 65
    g = _group(t, n, name)
    msgs, lists, valid, want = _walk_batch(t, n, name)
    assert len(msgs) == 7
    budget = 3 * t * _lib.RECW_TERM_BYTES[g.scheme_code in calls.G1_SIG_CODES]
    mb, buf, plen, m, stride = pack_partials(msgs, lists, g.scheme_code)
    out = {}
    for key, env in (("chunked", {"DGPU_RECOVER_WIDE_BUDGET": str(budget)}), ("whole", {"DGPU_RECOVER": "batched"})):
        with contextlib.closing(open_ctx(env)) as ctx:
            calls.set_group(ctx, g.scheme_code, t, n, g.commits)
            with calls.profiled(ctx) as stage_times:
                out[key] = [calls.recover_batch(ctx, mb, buf, plen, calls.sig_width(g.scheme_code), st)
                            for st in (False, True)]
                chunks = sorted(k for k in stage_times() if k.startswith("recover_msm_chunk"))
            want_chunks = ["recover_msm_chunk%d" % i for i in range(3)] if key == "chunked" else []
            assert chunks == want_chunks, (key, chunks)
    for a, b in zip(out["chunked"], out["whole"]):
        assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
        assert (a[2] is None and b[2] is None) or bytes(a[2]) == bytes(b[2])
    sigs, _ = _tg(g).recover_batch(msgs, lists, statuses=False)
    sl = len(want[1])
    assert [bytes(out["chunked"][0][0][sl * r:sl * (r + 1)]) if w else None for r, w in enumerate(want)] == want == sigs


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_generic_redo_paths(name):
    """DGPU_TEST_FORCE_EXC=1 (A/B build): the wide MSM kernels have no fast
    additions of their own (every addition is the generic one), the partial
    decoders' membership tests do -- the walk batch gives the same results."""
    t, n = 33, 65
    msgs, lists, valid, want = _walk_batch(t, n, name)
    with contextlib.closing(open_ctx({"DGPU_TEST_FORCE_EXC": "1"})) as ctx:
        grp = _tg(_group(t, n, name), ctx=ctx)
        assert grp.recover_batch(msgs, lists, statuses=False)[0] == want
        assert grp.recover_batch(msgs, lists, statuses=True) == (want, valid)


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_and_narrow_groups_take_turns(name):
    """A t = 17 group and a t = 33 group on one context, two turns each: each
    keeps its results.  dgpu_set_group_scheme with t = 33 still returns
    DGPU_EINVAL and leaves the wide group working."""
    from drand_amd import _lib, synth
    from drand_amd.threshold import ThresholdGroup
    wide = _group(33, 65, name)
    w_msgs, w_parts, w_want = _clean(33, 65, name)
    narrow = synth.make_group(77, 17, 32, scheme=wide.scheme_code)
    msgs, parts, ok = synth.make_recovery_batch(narrow, 3, seed=5, bad_rate=0.0)
    n_msgs = [bytes(x) for x in msgs]
    n_parts = [[bytes(p) for p in row] for row in parts]
    n_want = [bytes(s) for s in synth.group_signatures(narrow, msgs)]
    with contextlib.closing(open_ctx({})) as ctx:
        a = _tg(narrow, ctx=ctx)
        b = _tg(wide, ctx=ctx)
        for _ in range(2):
            assert a.recover_batch(n_msgs, n_parts, statuses=False)[0] == n_want
            assert b.recover_batch(w_msgs[:3], w_parts[:3], statuses=False)[0] == w_want[:3]
        buf = np.frombuffer(b"".join(wide.commits), dtype=np.uint8).copy()
        with ThresholdGroup._lock:
            b._install()
            assert ctx.lib.dgpu_set_group_scheme(ctx.handle, wide.scheme_code, 33, 65, _lib.ptr(buf),
                                                 len(wide.commits[0])) == _lib.DGPU_EINVAL
        assert b.recover_batch(w_msgs[:3], w_parts[:3])[0] == w_want[:3]


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_device_entry_point(name):
    """dgpu_recover_batch_device at (33, 65) on torch buffers, with d_status
    and a d_out that is not zero on entry."""
    import torch
    from drand_amd import calls
    from drand_amd.chain import get_context
    t, n = 33, 65
    g = _group(t, n, name)
    msgs, lists, valid, want = _walk_batch(t, n, name)
    sl = len(want[1])
    plen_full = 2 + sl
    nr, m = len(msgs), t + 2
    parts = np.zeros((nr, m, plen_full), dtype=np.uint8)
    plen = np.zeros((nr, m), dtype=np.int32)
    for r, row in enumerate(lists):
        for j, p in enumerate(row):
            parts[r, j, :len(p)] = np.frombuffer(p, dtype=np.uint8)
            plen[r, j] = len(p)
    ctx = get_context(0)
    calls.set_group(ctx, g.scheme_code, t, n, g.commits)
    dev = torch.device("cuda", 0)
    d_msgs = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(nr, 32).copy()).to(dev)
    d_parts = torch.from_numpy(parts).to(dev)
    d_plen = torch.from_numpy(plen).to(dev)
    d_out = torch.full((nr, sl), 0xA5, dtype=torch.uint8, device=dev)
    d_ok = torch.full((nr,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((nr * m,), 0xFF, dtype=torch.uint8, device=dev)
    calls.recover_batch_device(ctx, d_msgs, d_parts, d_plen, d_out, d_ok, d_st)
    torch.cuda.synchronize()
    ok = d_ok.cpu().numpy().astype(bool)
    out = d_out.cpu().numpy()
    st = d_st.cpu().numpy().reshape(nr, m)
    assert ok.tolist() == [w is not None for w in want]
    for r, w in enumerate(want):
        assert bytes(out[r]) == (w if w else bytes(sl)), r
        assert [s == 0 for s in st[r, :len(lists[r])]] == valid[r], r


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_multi_same_device_equals_single(name, monkeypatch):
    """MultiThresholdGroup over D = 2 contexts on one GPU at (33, 65) == the
    single-context result (two real ranks over RCCL: not measured here)."""
    from drand_amd.multi import MultiThresholdGroup
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    g = _group(33, 65, name)
    msgs, lists, valid, want = _walk_batch(33, 65, name)
    single = _tg(g).recover_batch(msgs, lists)
    mg = MultiThresholdGroup(g.commits, g.n, [0, 0], scheme=g.scheme_code)
    try:
        got = mg.recover_batch(msgs, lists)
        got_rlc = mg.recover_batch(msgs, lists, statuses=False)
    finally:
        mg.close()
    assert got == single == (want, valid)
    assert got_rlc[0] == want


# ---------------------------------------------------------------- past the walk's first 256 slots
# k_recover_walk_wide takes a round's slots in chunks of 256 and carries the
# good and distinct counts, the duplicate bitmap and the "more" flag from chunk
# to chunk.  m = 530 slots (three chunks) at (33, 65), most of them empty.
MANY_SLOTS = 530


@functools.lru_cache(maxsize=None)
def _many_slots_batch(name):
    from drand_amd import synth
    t, n, m = 33, 65, MANY_SLOTS
    g = _group(t, n, name)
    rng = np.random.default_rng(7)
    spread = list(range(0, 10)) + list(range(300, 316)) + list(range(520, 527))  # 33 slots over chunks 0, 1, 2
    assert len(spread) == t
    rows = []  # per round {slot: (signer, label)}
    sg = [list(map(int, rng.permutation(n))) for _ in range(6)]
    # 0: the t good ones spread over three chunks, the t-th in chunk 2, nothing after it: batched check
    rows.append({s: (sg[0][k], sg[0][k]) for k, s in enumerate(spread)})
    # 1: an invalid one in chunk 0, the t-th decodable in chunk 1, the only spare good one in chunk 2 (REC_MORE
    #    found in a later chunk): the batched check fails, the exact path walks on to the spare
    r1 = {s: (sg[1][k], sg[1][k]) for k, s in enumerate(list(range(0, 10)) + list(range(300, 323)))}
    r1[4] = (sg[1][4], (sg[1][4] + 1) % n if (sg[1][4] + 1) % n not in sg[1][:34] else sg[1][40])
    r1[525] = (sg[1][33], sg[1][33])
    rows.append(r1)
    # 2: a duplicate whose first occurrence sits in chunk 0 and whose second in chunk 1, a spare in chunk 2: the walk
    #    stops at t good with t - 1 distinct
    r2 = {s: (sg[2][k], sg[2][k]) for k, s in enumerate(spread[:t - 1])}
    r2[310] = (sg[2][3], sg[2][3])   # (slot 310 was signer 20's: now the signer of slot 3 again)
    r2[527] = (sg[2][40], sg[2][40])
    r2[528] = (sg[2][41], sg[2][41])
    rows.append(r2)
    # 3: t - 1 good ones after three chunks: short of t
    rows.append({s: (sg[3][k], sg[3][k]) for k, s in enumerate(spread[:t - 1])})
    # 4: as 2 but the duplicate is invalid (wrong signer under that label), so it does not count: t distinct good
    #    ones are reached with the spare in chunk 2 -- recovers through the exact path
    r4 = {s: (sg[4][k], sg[4][k]) for k, s in enumerate(spread[:t - 1])}
    r4[310] = (sg[4][50], sg[4][3])
    r4[527] = (sg[4][40], sg[4][40])
    r4[528] = (sg[4][41], sg[4][41])
    rows.append(r4)
    nr = len(rows)
    sidx = np.zeros((nr, m), dtype=np.uint32)
    lab = np.zeros((nr, m), dtype=np.uint32)
    for r, row in enumerate(rows):
        for s, (a, b) in row.items():
            sidx[r, s], lab[r, s] = a, b
    msgs = _msgs(nr, b"many")
    signed = synth.sign_partials(g, msgs, sidx, lab)
    lists, valid, slots = [], [], []
    for r, row in enumerate(rows):
        ps = [bytes(signed[r, s]) if s in row else b"" for s in range(m)]
        ok = [s in row and row[s][0] == row[s][1] for s in range(m)]
        lists.append(ps)
        valid.append(ok)
        slots.append([(row[s][1] if s in row else None, ok[s]) for s in range(m)])
    sigs = synth.group_signatures(g, msgs)
    want = [bytes(sigs[r]) if _reference_walk(t, slots[r]) else None for r in range(nr)]
    assert [w is not None for w in want] == [True, True, False, False, True]
    return [bytes(x) for x in msgs], lists, valid, want


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_walk_past_256_slots(name):
    """530 slots per round, three chunks of the walk kernel: the t-th good
    partial in a later chunk, a spare only in the last chunk, a duplicate
    across chunks, a round short of t after every chunk."""
    msgs, lists, valid, want = _many_slots_batch(name)
    grp = _tg(_group(33, 65, name))
    sigs, none = grp.recover_batch(msgs, lists, statuses=False)
    assert none is None and sigs == want
    sigs, got_valid = grp.recover_batch(msgs, lists, statuses=True)
    assert sigs == want
    assert got_valid == valid


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_gpu_wide_t257(name):
    """(257, 513), 2 rounds: the first threshold with 64 lanes per slice, two
    points per thread in the Lagrange kernel and a second chunk of the walk.
    Round 0 has t valid partials; round 1 has one under a wrong label."""
    from drand_amd import synth
    t, n = 257, 513
    g = _group(t, n, name)
    rng = np.random.default_rng(t)
    msgs = _msgs(2, b"t257")
    idx = np.argsort(rng.random((2, n)), axis=1)[:, :t].astype(np.uint32)
    lab = idx.copy()
    lab[1, 200] = idx[1, 200] + 1 if idx[1, 200] + 1 < n else 0
    parts = synth.sign_partials(g, msgs, idx, lab)
    want = [bytes(synth.group_signatures(g, msgs)[0]), None]
    lists = [[bytes(p) for p in row] for row in parts]
    grp = _tg(g)
    sigs, none = grp.recover_batch([bytes(x) for x in msgs], lists, statuses=False)
    assert none is None and sigs == want
    sigs, valid = grp.recover_batch([bytes(x) for x in msgs], lists, statuses=True)
    assert sigs == want
    assert valid == [[True] * t, [j != 200 for j in range(t)]]
