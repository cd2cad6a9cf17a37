"""tests/golden/keyed_identities.json is what its generator and the oracle
say: the hashes, two keys and two verdicts are re-derived here (CPU-only)."""
import hashlib
import importlib.util
import os

from conftest import GOLDEN, load_golden
from oracle import bls12381 as B


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_keyed", os.path.join(GOLDEN, "make_golden_keyed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shape_and_hashes():
    g = load_golden("keyed_identities.json")
    ids, g1s = g["identities"], g["g1_signatures"]
    assert len(ids["nodes"]) == 8 and ids["scheme"] == "pedersen-bls-chained"
    kinds = ["wrong_key", "sig_bit_flipped", "sig_infinity", "key_x_ge_p", "key_off_curve", "key_outside_subgroup",
             "key_identity"]
    for sec, klen, slen in ((ids, 48, 96), (g1s, 96, 48)):
        assert [m["kind"] for m in sec["mutations"]] == kinds
        for rec in sec["nodes"] + sec["mutations"]:
            key = bytes.fromhex(rec["key"])
            assert len(key) == klen and len(bytes.fromhex(rec["sig"])) == slen
            assert hashlib.blake2b(key, digest_size=32).hexdigest() == rec["hash"]
        by = {m["kind"]: m["reason"] for m in sec["mutations"]}
        assert by["wrong_key"] == 3 and by["sig_infinity"] == 4 and by["sig_bit_flipped"] in (1, 2)
        assert all(by[k] == 5 for k in kinds[3:])


def test_two_keys_and_two_verdicts_rederived():
    gen = _generator()
    g = load_golden("keyed_identities.json")["identities"]
    for i in (0, 5):
        assert B.sk_to_pk(gen.secret(b"g2sig/", i)).hex() == g["nodes"][i]["key"]
    n = g["nodes"][0]
    assert B.verify_g2(B.g1_decompress(bytes.fromhex(n["key"])), bytes.fromhex(n["hash"]), bytes.fromhex(n["sig"]))
    m = g["mutations"][0]  # node 0's signature under node 1's key
    assert m["sig"] == n["sig"] and m["key"] == g["nodes"][1]["key"]
    assert gen.reason(False, bytes.fromhex(m["key"]), bytes.fromhex(m["hash"]), bytes.fromhex(m["sig"]), B.DST_G2) == 3


def test_rejected_keys_are_rejected_by_the_oracle_decoders():
    g = load_golden("keyed_identities.json")
    for sec, dec in ((g["identities"], B.g1_decompress), (g["g1_signatures"], B.g2_decompress)):
        by = {m["kind"]: bytes.fromhex(m["key"]) for m in sec["mutations"]}
        for kind, word in (("key_x_ge_p", "x >= p"), ("key_off_curve", "not on curve"),
                           ("key_outside_subgroup", "not in subgroup")):
            try:
                dec(by[kind])
            except B.DecodeError as e:
                assert word in str(e), kind
            else:
                raise AssertionError(kind)
        dec(by["key_outside_subgroup"], check_subgroup=False)  # a curve point all the same
        assert dec(by["key_identity"]) is None
