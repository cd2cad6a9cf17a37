"""Generate the threshold-recovery fixtures of the G1-signature schemes
(tests/golden/recover_g1_*.json) from the oracle's primitives alone:

    python tests/golden/make_golden_recover_g1.py

A group is share_poly(seed, t) with commitments C_j = a_j g2 (sk_to_pk_g2);
PubPoly.Eval(i) = sum_j C_j (i+1)^j by Horner in G2; a partial is
BE16(index) || sign_g1(share, msg, dst); a partial is valid iff verify_g1
accepts it under Eval(index); recovery is kyber tbls.Recover's walk (first t
good in order, one per index, fewer than t distinct fails) followed by the
Lagrange combination in G1.  The DST is the scheme's: the G2 suite's for
bls-unchained-on-g1, the RFC 9380 G1 suite's for bls-unchained-g1-rfc9380.
Fixtures are data only (inputs + expected outputs).
"""
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import bls12381 as B  # noqa: E402
from oracle import drand_ref as D  # noqa: E402

SCHEME_DST = {"bls-unchained-on-g1": B.DST_G2, "bls-unchained-g1-rfc9380": B.DST_G1}
SCHEME_TAG = {"bls-unchained-on-g1": "on_g1", "bls-unchained-g1-rfc9380": "rfc9380"}
# (scheme, seed, t, n)
GROUPS = [("bls-unchained-on-g1", 3, 3, 8), ("bls-unchained-on-g1", 7, 12, 20), ("bls-unchained-on-g1", 5, 17, 32),
          ("bls-unchained-on-g1", 8, 32, 40), ("bls-unchained-g1-rfc9380", 3, 3, 8),
          ("bls-unchained-g1-rfc9380", 5, 17, 32)]


def fixture_name(scheme, t, n):
    return f"recover_g1_{SCHEME_TAG[scheme]}_t{t}_n{n}.json"


def eval_g2(commit_points, i):
    """PubPoly.Eval(i) in G2 (x_i = i + 1), Horner."""
    acc = None
    for c in reversed(commit_points):
        acc = B.g2_add(B.g2_mul(acc, i + 1) if acc is not None else None, c)
    return acc


def off_subgroup_point():
    """A compressed point on E1 outside the r-order subgroup: the first x >= 1
    whose point decodes without the subgroup check and fails with it."""
    x = 1
    while True:
        data = bytearray(x.to_bytes(48, "big"))
        data[0] |= 0x80
        try:
            B.g1_decompress(bytes(data), check_subgroup=False)
        except B.DecodeError:
            x += 1
            continue
        try:
            B.g1_decompress(bytes(data))
        except B.DecodeError:
            return bytes(data)
        x += 1


def recover_walk(msg, partials, valid, t):
    """tbls.Recover (R) given the VerifyPartial verdicts."""
    good = []
    for s, v in zip(partials, valid):
        if not v:
            continue
        good.append((struct.unpack(">H", s[:2])[0], B.g1_decompress(s[2:])))
        if len(good) >= t:
            break
    pts = {}
    for idx, pt in sorted(good, key=lambda p: p[0]):
        pts.setdefault(idx, pt)
    if len(pts) < t:
        return None
    order = sorted(pts)
    lam = D.lagrange_at_zero([i + 1 for i in order])
    acc = None
    for i, l in zip(order, lam):
        acc = B.g1_add(acc, B.g1_mul(pts[i], l))
    return B.g1_compress(acc)


def recover_cases_g1(scheme, seed, t, n):
    dst = SCHEME_DST[scheme]
    rng = random.Random(seed)
    co = D.share_poly(seed, t)
    commits = [B.sk_to_pk_g2(a) for a in co]
    cpts = [B.g2_decompress(c) for c in commits]
    sig_of = lambda i, m: struct.pack(">H", i) + B.sign_g1(D.poly_eval(co, i + 1), m, dst)  # noqa: E731
    cases = []

    def add(kind, msg, partials):
        valid = []
        for s in partials:
            if len(s) < 2:
                valid.append(False)
                continue
            idx = struct.unpack(">H", s[:2])[0]
            valid.append(bool(B.verify_g1(eval_g2(cpts, idx), msg, s[2:], dst)))
        rec = recover_walk(msg, partials, valid, t)
        if rec is not None:
            assert rec == B.sign_g1(co[0], msg, dst) and B.verify_g1(cpts[0], msg, rec, dst)
        cases.append({"kind": kind, "msg": msg.hex(), "partials": [x.hex() for x in partials], "valid": valid,
                      "recovered": rec.hex() if rec else None})
        print(scheme, t, kind, sum(valid), "valid", "ok" if rec else "fail", flush=True)

    def msg(k):
        return hashlib.sha256(b"drand-mi355x/recover-g1/" + bytes([seed, k])).digest()

    m = msg(0)
    idx = rng.sample(range(n), t)
    add("exact_t", m, [sig_of(i, m) for i in idx])
    m = msg(1)
    idx = rng.sample(range(n), t + 3)
    ps = [sig_of(i, m) for i in idx]
    ps[1] = sig_of(idx[1], msg(9))                         # signature of another message
    b = bytearray(ps[3]); b[10] ^= 0x04; ps[3] = bytes(b)  # bit flip in x
    ps[4] = struct.pack(">H", idx[5]) + ps[4][2:]          # valid sig under the wrong index
    add("three_bad_enough", m, ps)
    m = msg(2)
    idx = rng.sample(range(n), t)
    ps = [sig_of(i, m) for i in idx]
    ps[t // 2] = sig_of(idx[t // 2], msg(8))
    add("one_bad_short", m, ps)
    m = msg(3)
    idx = rng.sample(range(n), t + 1)
    ps = [sig_of(i, m) for i in idx]
    ps.insert(1, ps[0])                                    # duplicate index among the first t good
    add("duplicate_index", m, ps)
    m = msg(4)
    idx = rng.sample(range(n), t)
    ps = [b"", b"\x00"] + [sig_of(i, m) for i in idx] + [sig_of(n + 7, m)]
    add("short_partials_and_extra", m, ps)
    m = msg(5)
    idx = rng.sample(range(n), t - 1)
    ps = [sig_of(i, m) for i in idx] + [sig_of(n + 3, m)]  # a share index beyond n (Eval(i) is defined for any i)
    add("index_beyond_n", m, ps)
    m = msg(6)
    idx = rng.sample(range(n), t + 2)
    ps = [sig_of(i, m) for i in idx]
    ps[0] = ps[0][:2] + bytes([0xC0]) + bytes(47)          # the compressed point at infinity
    add("infinity_partial", m, ps[:t + 1])
    m = msg(7)
    ps = [sig_of(i, m) for i in idx]
    ps[1] = ps[1][:2] + off_subgroup_point()               # on the curve, outside the subgroup
    add("off_subgroup_partial", m, ps[:t + 1])
    name = fixture_name(scheme, t, n)
    with open(os.path.join(HERE, name), "w") as f:
        json.dump({"source": "kyber tbls.Recover (R) over oracle/bls12381 sign_g1 / verify_g1 and a G2 public polynomial",
                   "scheme": scheme, "dst": dst.decode(), "seed": seed, "t": t, "n": n,
                   "commits": [c.hex() for c in commits], "group_sig_of": "sk = a_0 = drand_ref.share_poly(seed)[0]",
                   "cases": cases}, f, indent=1, sort_keys=True)
    print("wrote", name, flush=True)


if __name__ == "__main__":
    want = sys.argv[1:]
    for scheme, seed, t, n in GROUPS:
        if not want or fixture_name(scheme, t, n) in want:
            recover_cases_g1(scheme, seed, t, n)
