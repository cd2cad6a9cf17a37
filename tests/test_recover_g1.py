"""Threshold recovery for the G1-signature schemes (bls-unchained-on-g1,
bls-unchained-g1-rfc9380): the same kyber tbls.Recover / VerifyPartial call
sites (chain/beacon/chain.go:158-168, node.go:117-125) with the signature
group G1 and the public polynomial in G2.

CPU: the new C-ABI entry points are declared, bound and exported; the
fixtures (tests/golden/make_golden_recover_g1.py, composed from the oracle's
sign_g1 / verify_g1 and a Horner Eval in G2) recover the group secret's
signature; ThresholdGroup rejects commitments that do not fit the scheme
before touching the library.  GPU: every fixture bit-exactly on the exact
per-partial path and on the batched check, reason codes, a 197-round
property batch, the synthetic-partial tool, group switching on one context,
error paths, the stage count and the multi-device loopback."""
import contextlib
import ctypes
import hashlib
import os
import re
import struct

import pytest

from conftest import ROOT, load_golden
from oracle import bls12381 as B
from oracle import drand_ref as D

# t = 3, 12, 17, 32 under the G2-suite DST, t = 3, 17 under the RFC 9380 G1 DST
FIXTURES = ["recover_g1_on_g1_t3_n8.json", "recover_g1_on_g1_t12_n20.json", "recover_g1_on_g1_t17_n32.json",
            "recover_g1_on_g1_t32_n40.json", "recover_g1_rfc9380_t3_n8.json", "recover_g1_rfc9380_t17_n32.json"]
DSTS = {"bls-unchained-on-g1": B.DST_G2, "bls-unchained-g1-rfc9380": B.DST_G1}
NEW_ENTRY_POINTS = {
    "dgpu_set_group_scheme": (ctypes.c_int, 6),
    "dgpu_make_partials_scheme": (ctypes.c_int, 10),
    "dgpu_multi_set_group_scheme": (ctypes.c_int, 6),
}
KINDS = ["exact_t", "three_bad_enough", "one_bad_short", "duplicate_index", "short_partials_and_extra",
         "index_beyond_n", "infinity_partial", "off_subgroup_partial"]


def _batch(g):
    msgs = [bytes.fromhex(c["msg"]) for c in g["cases"]]
    parts = [[bytes.fromhex(p) for p in c["partials"]] for c in g["cases"]]
    return msgs, parts


def _group(g, **kw):
    from drand_amd.threshold import ThresholdGroup
    return ThresholdGroup([bytes.fromhex(c) for c in g["commits"]], g["n"], scheme=g["scheme"], **kw)


# ---------------------------------------------------------------- CPU
def test_new_entry_points_declared_bound_and_exported():
    """include/drand_gpu.h declares the scheme-aware group, partial-tool and
    multi entry points, _lib binds them with matching signatures and
    libdrand_gpu.so exports them (ABI 3, additive)."""
    from drand_amd import _lib
    with open(os.path.join(ROOT, "include", "drand_gpu.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, nargs) in NEW_ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name + " not declared"
        assert len(decl.group(1).split(",")) == nargs, name
        assert name in bound, name + " not bound"
        assert bound[name][0] is res and len(bound[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    sg = bound["dgpu_set_group_scheme"][1]
    assert sg[1:4] == [ctypes.c_int] * 3 and sg[5] is ctypes.c_size_t
    assert bound["dgpu_multi_set_group_scheme"][1][1:] == sg[1:]
    mp = bound["dgpu_make_partials_scheme"][1]
    assert mp[1] is ctypes.c_int and mp[2] is ctypes.c_size_t and mp[4] is ctypes.c_size_t
    assert "out_sigs96" not in header and lib.dgpu_abi_version() == 3 == _lib.ABI_VERSION


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_recovered_is_group_signature(name):
    g = load_golden(name)
    dst = DSTS[g["scheme"]]
    assert g["dst"] == dst.decode()
    co = D.share_poly(g["seed"], g["t"])
    assert [bytes.fromhex(c) for c in g["commits"]] == [B.sk_to_pk_g2(a) for a in co]
    kinds = {c["kind"]: c for c in g["cases"]}
    assert list(kinds) == KINDS
    assert kinds["exact_t"]["recovered"] and kinds["one_bad_short"]["recovered"] is None
    assert kinds["duplicate_index"]["recovered"] is None  # kyber stops at t good, duplicates count once
    assert kinds["infinity_partial"]["valid"][0] is False and kinds["infinity_partial"]["recovered"]
    assert kinds["off_subgroup_partial"]["valid"][1] is False and kinds["off_subgroup_partial"]["recovered"]
    inf, off = (bytes.fromhex(kinds[k]["partials"][j])[2:] for k, j in (("infinity_partial", 0),
                                                                        ("off_subgroup_partial", 1)))
    assert B.g1_decompress(inf) is None
    assert B.g1_decompress(off, check_subgroup=False) is not None
    with pytest.raises(B.DecodeError):
        B.g1_decompress(off)
    for c in g["cases"]:
        assert all(len(bytes.fromhex(p)) in (0, 1, 50) for p in c["partials"])
        if c["recovered"] is not None:
            assert bytes.fromhex(c["recovered"]) == B.sign_g1(co[0], bytes.fromhex(c["msg"]), dst)


def test_fixture_partial_verifies_under_g2_eval():
    """One real VerifyPartial of the oracle per DST: a fixture partial verifies
    under Eval(index) in G2 and under no other index."""
    for name in ("recover_g1_on_g1_t3_n8.json", "recover_g1_rfc9380_t3_n8.json"):
        g = load_golden(name)
        cpts = [B.g2_decompress(bytes.fromhex(c)) for c in g["commits"]]
        c = g["cases"][0]
        p = bytes.fromhex(c["partials"][0])
        idx = struct.unpack(">H", p[:2])[0]

        def ev(i):
            acc = None
            for cj in reversed(cpts):
                acc = B.g2_add(B.g2_mul(acc, i + 1) if acc is not None else None, cj)
            return acc
        assert B.verify_g1(ev(idx), bytes.fromhex(c["msg"]), p[2:], DSTS[g["scheme"]])
        assert not B.verify_g1(ev(idx + 1), bytes.fromhex(c["msg"]), p[2:], DSTS[g["scheme"]])


def test_threshold_group_argument_validation(monkeypatch):
    """A commitment length that does not fit the scheme raises ValueError
    before any library call (no GPU, no context)."""
    from drand_amd import _lib, threshold
    from drand_amd.scheme import get_scheme_by_id_with_default

    def no_context(*a, **k):
        raise AssertionError("library touched")
    monkeypatch.setattr(threshold, "get_context", no_context)
    g1c, g2c = [bytes(48)] * 3, [bytes(96)] * 3
    with pytest.raises(ValueError):
        threshold.ThresholdGroup(g2c, 8)
    for scheme in ("bls-unchained-on-g1", _lib.SCHEME_G1_RFC9380, get_scheme_by_id_with_default("bls-unchained-on-g1")):
        with pytest.raises(ValueError):
            threshold.ThresholdGroup(g1c, 8, scheme=scheme)
    for scheme in ("pedersen-bls-chained", _lib.SCHEME_UNCHAINED, None):
        with pytest.raises(ValueError):
            threshold.ThresholdGroup(g2c, 8, scheme=scheme)
    with pytest.raises(ValueError):
        threshold.ThresholdGroup(g2c, 8, scheme="no-such-scheme")
    with pytest.raises(ValueError):
        threshold.ThresholdGroup(g2c, 8, scheme=7)
    with pytest.raises(ValueError):
        threshold.ThresholdGroup([bytes(96), bytes(48)], 8, scheme="bls-unchained-on-g1")
    assert threshold.group_scheme_code(g2c, "bls-unchained-g1-rfc9380") == _lib.SCHEME_G1_RFC9380
    assert threshold.group_scheme_code(g1c) == _lib.SCHEME_CHAINED
    mb, buf, plen, m, stride = threshold.pack_partials([bytes(32)], [[b"ab"]], _lib.SCHEME_UNCHAINED_G1)
    assert stride == 50 and threshold.pack_partials([bytes(32)], [[b"ab"]])[4] == 98


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_recover_g1_exact_path_matches_fixtures(name):
    g = load_golden(name)
    msgs, parts = _batch(g)
    sigs, valid = _group(g).recover_batch(msgs, parts)
    for c, s, v in zip(g["cases"], sigs, valid):
        assert v == c["valid"], c["kind"]
        assert (s.hex() if s else None) == c["recovered"], c["kind"]
        assert s is None or len(s) == 48


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_recover_g1_batched_check_matches_fixtures(name):
    """statuses=False: one pairing per round over the first t decodable
    partials, the undecided rounds (three_bad_enough has more decodable
    partials left) down the exact path."""
    g = load_golden(name)
    msgs, parts = _batch(g)
    sigs, valid = _group(g).recover_batch(msgs, parts, statuses=False)
    assert valid is None
    assert [s.hex() if s else None for s in sigs] == [c["recovered"] for c in g["cases"]]


def _expected_reason(partial, valid):
    from drand_amd import _lib
    if valid:
        return _lib.REASON_OK
    if len(partial) != 50:
        return _lib.REASON_DECODE
    try:
        pt = B.g1_decompress(partial[2:], check_subgroup=False)
    except B.DecodeError:
        return _lib.REASON_DECODE
    if pt is None:
        return _lib.REASON_INFINITY
    try:
        B.g1_decompress(partial[2:])
    except B.DecodeError:
        return _lib.REASON_SUBGROUP
    return _lib.REASON_PAIRING


@pytest.mark.gpu
def test_gpu_recover_g1_reason_codes_device_entry_point():
    """dgpu_recover_batch_device's d_status on the t = 3 fixture plus a round
    that offers a 98-byte (G2-signature) partial to the G1 group."""
    import numpy as np
    import torch
    from drand_amd import _lib, calls
    from drand_amd.threshold import pack_partials
    g = load_golden("recover_g1_on_g1_t3_n8.json")
    msgs, parts = _batch(g)
    g2part = bytes.fromhex(load_golden("recover_t3_n8.json")["cases"][0]["partials"][0])
    assert len(g2part) == 98
    msgs.append(msgs[0])
    parts.append([g2part] + parts[0])
    valid = [list(c["valid"]) for c in g["cases"]] + [[False] + list(g["cases"][0]["valid"])]
    recovered = [c["recovered"] for c in g["cases"]] + [g["cases"][0]["recovered"]]
    grp = _group(g)
    mb, buf, plen, m, stride = pack_partials(msgs, parts, grp.scheme_code)
    assert stride == 98  # the stride follows the longest partial offered
    nr = len(msgs)
    dev = torch.device("cuda", 0)
    d_msgs = torch.from_numpy(mb).to(dev)
    d_parts = torch.from_numpy(buf).to(dev)
    d_plen = torch.from_numpy(plen.astype(np.int32)).to(dev)
    d_out = torch.full((nr, 48), 0xEE, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(nr, dtype=torch.uint8, device=dev)
    d_st = torch.full((nr * m,), 0xFF, dtype=torch.uint8, device=dev)
    from drand_amd.threshold import ThresholdGroup
    with ThresholdGroup._lock:
        grp._install()
        calls.recover_batch_device(grp.ctx, d_msgs, d_parts, d_plen, d_out, d_ok, d_st)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy().reshape(nr, m)
    out = d_out.cpu().numpy()
    ok = d_ok.cpu().numpy()
    for r in range(nr):
        want = [_expected_reason(p, v) for p, v in zip(parts[r], valid[r])]
        assert st[r, :len(want)].tolist() == want, r
        assert st[r, len(want):].tolist() == [_lib.REASON_DECODE] * (m - len(want))  # empty slots
        assert bool(ok[r]) == (recovered[r] is not None)
        assert bytes(out[r]).hex() == (recovered[r] or bytes(48).hex())
    k = {c["kind"]: i for i, c in enumerate(g["cases"])}
    assert st[k["infinity_partial"], 0] == _lib.REASON_INFINITY
    assert st[k["off_subgroup_partial"], 1] == _lib.REASON_SUBGROUP
    assert st[k["short_partials_and_extra"], :2].tolist() == [_lib.REASON_DECODE] * 2
    assert st[nr - 1, 0] == _lib.REASON_DECODE                 # the 98-byte partial
    assert st[k["three_bad_enough"], 4] == _lib.REASON_PAIRING  # valid signature under the wrong index
    assert st[k["three_bad_enough"], 1] == _lib.REASON_PAIRING  # signature of another message


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["bls-unchained-on-g1", "bls-unchained-g1-rfc9380"])
def test_gpu_recover_g1_property_batch(scheme):
    """197 rounds (no multiple of 64 or 8), t = 5 of n = 9, m = 7 slots with
    empty ones, rounds alternating t and t - 1 good partials, both modes."""
    import numpy as np
    from drand_amd import synth
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    from drand_amd.threshold import ThresholdGroup
    code = scheme_code(get_scheme_by_id_with_default(scheme))
    t, n, nr, m = 5, 9, 197, 7
    grp = synth.make_group(11, t, n, scheme=code)
    co = D.share_poly(11, t)
    assert grp.commits == [B.sk_to_pk_g2(a) for a in co]
    rng = np.random.default_rng(4)
    msgs = np.stack([np.frombuffer(hashlib.sha256(b"g1 round" + struct.pack(">I", r)).digest(), dtype=np.uint8)
                     for r in range(nr)])
    sign_idx = np.argsort(rng.random((nr, n)), axis=1)[:, :t].astype(np.uint32)
    signed = synth.sign_partials(grp, msgs, sign_idx)
    assert signed.shape == (nr, t, 50)
    expect = synth.group_signatures(grp, msgs)
    assert expect.shape == (nr, 48)
    for r in (0, 98, 196):
        assert bytes(expect[r]) == B.sign_g1(co[0], bytes(msgs[r]), DSTS[scheme])
    parts, want = [], []
    for r in range(nr):
        k = t if r % 2 == 0 else t - 1
        p = [bytes(signed[r, j]) for j in range(k)]
        slots = [p[0], b"", p[1], p[2], b"", p[3]] + ([p[4]] if k == t else [b""])
        assert len(slots) == m
        parts.append(slots)
        want.append(bytes(expect[r]) if k == t else None)
    tg = ThresholdGroup(grp.commits, n, scheme=scheme)
    mlist = [bytes(x) for x in msgs]
    sigs, valid = tg.recover_batch(mlist, parts, statuses=True)
    assert sigs == want
    assert valid == [[len(s) == 50 for s in row] for row in parts]
    sigs, valid = tg.recover_batch(mlist, parts, statuses=False)
    assert sigs == want and valid is None


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["bls-unchained-on-g1", "bls-unchained-g1-rfc9380"])
def test_gpu_make_partials_scheme_matches_oracle(scheme):
    """dgpu_make_partials_scheme == BE16(label) || sign_g1(share, msg, dst) on
    a 2 x 3 sample; commitments derived on the GPU == sk_to_pk_g2."""
    import numpy as np
    from drand_amd import synth
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    code = scheme_code(get_scheme_by_id_with_default(scheme))
    grp = synth.make_group(9, 3, 5, scheme=code)
    co = D.share_poly(9, 3)
    assert grp.commits == [B.sk_to_pk_g2(a) for a in co]
    msgs = np.stack([np.frombuffer(hashlib.sha256(bytes([k])).digest(), dtype=np.uint8) for k in range(2)])
    idx = np.array([[0, 4, 2], [3, 1, 0]], dtype=np.uint32)
    lab = idx.copy()
    lab[1, 2] = 2
    parts = synth.sign_partials(grp, msgs, idx, lab)
    assert parts.shape == (2, 3, 50)
    for r in range(2):
        for j in range(3):
            sig = B.sign_g1(D.poly_eval(co, int(idx[r, j]) + 1), bytes(msgs[r]), DSTS[scheme])
            assert bytes(parts[r, j]) == struct.pack(">H", int(lab[r, j])) + sig


@pytest.mark.gpu
def test_gpu_group_switching_on_one_context():
    """G2-signature group, G1-signature group, the first again, then beacon
    verification under an on-G1 key: one context, nothing interferes (the
    group's C_0 line table lives outside the key cache)."""
    from drand_amd.chain import Beacon, Verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.threshold import ThresholdGroup
    ch = load_golden("chain_on_g1_s1.json")
    v = Verifier(get_scheme_by_id_with_default("bls-unchained-on-g1"), device=0)
    beacons = [Beacon(bytes.fromhex(r["prev"]), r["round"], bytes.fromhex(r["sig"])) for r in ch["rounds"][:4]]
    beacons += [Beacon(bytes.fromhex(c["prev"]), c["round"], bytes.fromhex(c["sig"])) for c in ch["corrupted"][:4]]
    pk = bytes.fromhex(ch["pk"])
    before = v.verify_reasons(beacons, pk).tolist()
    assert before[:4] == [0] * 4 and all(before[4:])
    g2 = load_golden("recover_t3_n8.json")
    g1 = load_golden("recover_g1_on_g1_t3_n8.json")
    grp2 = ThresholdGroup([bytes.fromhex(c) for c in g2["commits"]], g2["n"])
    grp1 = _group(g1)
    assert grp1.ctx is grp2.ctx is v.ctx
    first = grp2.recover_batch(*_batch(g2))
    assert [s.hex() if s else None for s in first[0]] == [c["recovered"] for c in g2["cases"]]
    got = grp1.recover_batch(*_batch(g1))
    assert [s.hex() if s else None for s in got[0]] == [c["recovered"] for c in g1["cases"]]
    assert got[1] == [c["valid"] for c in g1["cases"]]
    assert grp2.recover_batch(*_batch(g2)) == first
    assert grp1.recover_batch(*_batch(g1), statuses=False)[0] == got[0]
    assert v.verify_reasons(beacons, pk).tolist() == before


@pytest.mark.gpu
def test_gpu_set_group_scheme_error_paths_keep_the_group():
    import numpy as np
    from drand_amd import _lib
    from drand_amd.threshold import ThresholdGroup
    g = load_golden("recover_g1_rfc9380_t3_n8.json")
    grp = _group(g)
    msgs, parts = _batch(g)
    want = [c["recovered"] for c in g["cases"]]
    lib, h = grp.ctx.lib, grp.ctx.handle
    commits = b"".join(bytes.fromhex(c) for c in g["commits"])
    good = np.frombuffer(commits, dtype=np.uint8).copy()
    flipped = good.copy()
    flipped[96 + 40] ^= 0x10
    big = np.frombuffer(commits * 11, dtype=np.uint8).copy()
    code = grp.scheme_code

    def still_works():
        sigs, _ = grp.recover_batch(msgs, parts, statuses=False)
        assert [s.hex() if s else None for s in sigs] == want

    with ThresholdGroup._lock:
        grp._install()
        assert lib.dgpu_set_group_scheme(h, code, 3, 8, _lib.ptr(good), 48) == _lib.DGPU_EINVAL
        assert lib.dgpu_set_group_scheme(h, _lib.SCHEME_CHAINED, 3, 8, _lib.ptr(good), 96) == _lib.DGPU_EINVAL
        assert lib.dgpu_set_group_scheme(h, 9, 3, 8, _lib.ptr(good), 96) == _lib.DGPU_EINVAL
    still_works()
    with ThresholdGroup._lock:
        assert lib.dgpu_set_group_scheme(h, code, 3, 8, _lib.ptr(flipped), 96) == _lib.DGPU_EINVAL
    still_works()
    with ThresholdGroup._lock:
        assert lib.dgpu_set_group_scheme(h, code, 33, 40, _lib.ptr(big), 96) == _lib.DGPU_EINVAL
        assert lib.dgpu_set_group_scheme(h, code, 3, 2, _lib.ptr(good), 96) == _lib.DGPU_EINVAL
    still_works()


@pytest.mark.gpu
def test_gpu_recover_g1_stage_count_within_max_stages():
    from drand_amd import _lib, calls
    g = load_golden("recover_g1_on_g1_t17_n32.json")
    grp = _group(g)
    msgs, parts = _batch(g)
    with calls.profiled(grp.ctx) as stage_times:
        for statuses in (True, False):
            grp.recover_batch(msgs, parts, statuses=statuses)
            st = stage_times()
            assert 8 < len(st) <= _lib.MAX_STAGES, st
            assert "recover_msm" in st and "eng_lines" in st


@pytest.mark.gpu
@pytest.mark.parametrize("statuses", [True, False])
def test_gpu_recover_g1_library_defaults(statuses):
    """The shipped thresholds (the suite lowers them, conftest.py): a small
    call takes the Granger-Scott final exponentiation and the lane kernels'
    size class; the G1 form's lines kernel serves every size."""
    from conftest import open_ctx
    from drand_amd import _lib
    from drand_amd.threshold import ThresholdGroup
    g = load_golden("recover_g1_rfc9380_t17_n32.json")
    msgs, parts = _batch(g)
    assert len(g["commits"]) == g["t"]
    with contextlib.closing(open_ctx({"DGPU_THR_MIN": "65536", "DGPU_FE_GS_MAX": "16384", "DGPU_COF_ENGINE_MAX": "16384"})) as ctx:
        grp = ThresholdGroup([bytes.fromhex(c) for c in g["commits"]], g["n"], scheme=_lib.SCHEME_G1_RFC9380, ctx=ctx)
        sigs, valid = grp.recover_batch(msgs, parts, statuses=statuses)
    assert [s.hex() if s else None for s in sigs] == [c["recovered"] for c in g["cases"]]
    if statuses:
        assert valid == [c["valid"] for c in g["cases"]]


@pytest.mark.gpu
def test_gpu_recover_g1_multi_same_device_equals_single(monkeypatch):
    """D = 2 contexts on one GPU, the 17/32 fixture padded to 21 rounds
    (shards 16 + 5): dgpu_recover_multi == the single-context call."""
    from drand_amd.multi import MultiThresholdGroup
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    g = load_golden("recover_g1_on_g1_t17_n32.json")
    msgs, parts = _batch(g)
    msgs, parts = (msgs * 3)[:21], (parts * 3)[:21]
    single = _group(g).recover_batch(msgs, parts)
    mg = MultiThresholdGroup([bytes.fromhex(c) for c in g["commits"]], g["n"], [0, 0], scheme=g["scheme"])
    try:
        got = mg.recover_batch(msgs, parts)
        got_rlc = mg.recover_batch(msgs, parts, statuses=False)
    finally:
        mg.close()
    assert got == single
    assert got_rlc[0] == single[0]
    assert [s.hex() if s else None for s in got[0]] == ([c["recovered"] for c in g["cases"]] * 3)[:21]
