"""Generate tests/golden/keyed_identities.json from the oracle
(oracle/bls12381.py): node identities as key/keys.go:52-63 checks them --
AuthScheme.Verify(Key, blake2b-256(Key), Signature), signatures on G2 and
keys on G1 -- and the same shape under a G1-signature scheme (keys on G2),
each with mutated records and the reason the oracle gives them.

    python tests/golden/make_golden_keyed.py

A record's reason: 5 (DGPU_REASON_KEY) when the oracle's key decode rejects
the key or yields the identity -- the reference decodes the key first --,
else the signature's own decode / pairing reason (verify_g2 / verify_g1 and
their decoders).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import bls12381 as B  # noqa: E402

REASON_KEY = 5


def secret(tag, i):
    return int.from_bytes(hashlib.sha256(b"drand-mi355x/keyed/" + tag + bytes([i])).digest(), "big") % B.R


def ident_hash(key):
    return hashlib.blake2b(key, digest_size=32).digest()


def reason(g1sig, key, msg, sig, dst):
    """Key first, then the signature: decode, subgroup, identity, pairing."""
    try:
        kp = (B.g2_decompress if g1sig else B.g1_decompress)(key)
    except B.DecodeError:
        return REASON_KEY
    if kp is None:
        return REASON_KEY
    try:
        sp = (B.g1_decompress if g1sig else B.g2_decompress)(sig)
    except B.DecodeError as e:
        return 2 if "subgroup" in str(e) else 1
    if sp is None:
        return 4
    ok = B.verify_g1(kp, msg, sig, dst) if g1sig else B.verify_g2(kp, msg, sig, dst)
    return 0 if ok else 3


def bad_keys(g1sig):
    """Compressed keys the decoder must reject: x >= p, x not on the curve, a
    curve point outside the r-order subgroup, the identity."""
    n = 96 if g1sig else 48
    out = {}
    xp = bytearray((B.P + 1).to_bytes(48, "big") + (bytes(48) if g1sig else b""))
    xp[0] |= 0x80
    out["key_x_ge_p"] = bytes(xp)
    off = sub = None
    x = 1
    while off is None or sub is None:
        x += 1
        # (a G2 point is encoded c1 || c0: x = (x, 0))
        enc = bytearray(bytes(48) + x.to_bytes(48, "big")) if g1sig else bytearray(x.to_bytes(48, "big"))
        enc[0] |= 0x80
        try:
            (B.g2_decompress if g1sig else B.g1_decompress)(bytes(enc), check_subgroup=False)
        except B.DecodeError:
            off = off or bytes(enc)
            continue
        try:
            (B.g2_decompress if g1sig else B.g1_decompress)(bytes(enc))
        except B.DecodeError:
            sub = sub or bytes(enc)
    out["key_off_curve"] = off
    out["key_outside_subgroup"] = sub
    out["key_identity"] = bytes([0xC0]) + bytes(n - 1)
    return out


def section(g1sig, count, dst):
    tag = b"g1sig/" if g1sig else b"g2sig/"
    nodes = []
    for i in range(count):
        sk = secret(tag, i)
        key = B.sk_to_pk_g2(sk) if g1sig else B.sk_to_pk(sk)
        msg = ident_hash(key)
        sig = B.sign_g1(sk, msg, dst) if g1sig else B.sign_g2(sk, msg, dst)
        assert reason(g1sig, key, msg, sig, dst) == 0
        nodes.append({"key": key.hex(), "hash": msg.hex(), "sig": sig.hex()})
    k = [bytes.fromhex(n["key"]) for n in nodes]
    s = [bytes.fromhex(n["sig"]) for n in nodes]
    flipped = bytearray(s[1])
    flipped[-1] ^= 1
    sig_len = 48 if g1sig else 96
    muts = [("wrong_key", k[1], s[0]), ("sig_bit_flipped", k[1], bytes(flipped)),
            ("sig_infinity", k[2], bytes([0xC0]) + bytes(sig_len - 1))]
    muts += [(kind, key, s[3 % count]) for kind, key in bad_keys(g1sig).items()]
    out = []
    for kind, key, sig in muts:
        msg = ident_hash(key)
        out.append({"kind": kind, "key": key.hex(), "hash": msg.hex(), "sig": sig.hex(),
                    "reason": reason(g1sig, key, msg, sig, dst)})
    return {"nodes": nodes, "mutations": out}


def main():
    doc = {"source": "oracle/bls12381.py; key/keys.go:52-63, key/group.go:27,474-482",
           "hash": "blake2b-256 of the compressed key",
           "identities": dict(scheme="pedersen-bls-chained", **section(False, 8, B.DST_G2)),
           "g1_signatures": dict(scheme="bls-unchained-g1-rfc9380", **section(True, 3, B.DST_G1))}
    with open(os.path.join(HERE, "keyed_identities.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote keyed_identities.json")


if __name__ == "__main__":
    main()
