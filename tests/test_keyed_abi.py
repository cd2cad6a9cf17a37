"""The per-record-key entry points at the ABI: the header declares them, the
binding lists them with as many arguments, the library exports them, the ABI
version is still 3, and the Python wrappers pack their arguments as the header
says.  CPU-only."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_abi import declared_params as _declared_params

NAMES = {"dgpu_verify_keyed": 17, "dgpu_verify_keyed_device": 18, "dgpu_verify_partials": 11,
         "dgpu_verify_partials_device": 12}


def _header():
    return open(os.path.join(ROOT, "include", "drand_gpu.h")).read()


def test_header_declares_the_entry_points_and_the_reason():
    for name, count in NAMES.items():
        assert len(_declared_params(name)) == count, name
    host = [p.split()[-1].lstrip("*") for p in _declared_params("dgpu_verify_keyed")]
    assert host == ["ctx", "scheme", "n_keys", "keys", "key_len", "n", "key_idx", "msgs", "msg_stride", "msg_len",
                    "sigs", "sig_stride", "sig_len", "mode", "rlc_seed", "verdict_bits", "reason"]
    assert _declared_params("dgpu_verify_keyed_device")[-1].split()[-1].lstrip("*") == "stream"
    assert _declared_params("dgpu_verify_partials_device")[-1].split()[-1].lstrip("*") == "stream"
    assert re.search(r"DGPU_REASON_KEY = 5\b", _header())
    assert re.search(r"#define DGPU_ABI_VERSION 3\b", _header())


def test_binding_matches_the_header():
    from drand_amd import _lib
    assert _lib.REASON_KEY == 5
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NAMES:
        res, args = bound[name]
        assert res is _lib.ctypes.c_int and len(args) == len(_declared_params(name)), name
    for name in ("dgpu_verify_keyed", "dgpu_verify_keyed_device"):
        args = bound[name][1]
        assert [args[i] for i in (2, 4, 5, 8, 11)] == [_lib.ctypes.c_size_t] * 5 and args[14] is _lib.ctypes.c_uint64
    for name in ("dgpu_verify_partials", "dgpu_verify_partials_device"):
        assert bound[name][1][8] is _lib.ctypes.c_uint64


def test_library_exports_them():
    from drand_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.dgpu_abi_version() == 3


def test_pack_keyed_on_empty_and_one_record_inputs():
    from drand_amd import _lib, chain
    key = bytes([0x80]) + bytes(47)
    kb, key_len, idx, mb, ml, sb, sl = chain.pack_keyed(_lib.SCHEME_CHAINED, [key], [], [], [])
    assert (kb.size, key_len, idx.size, ml.size, sl.size) == (48, 48, 0, 0, 0) and idx.dtype == np.uint32
    kb, key_len, idx, mb, ml, sb, sl = chain.pack_keyed(_lib.SCHEME_CHAINED, [key, key], [1], [b"abc"], [b"\x01" * 5])
    assert kb.tobytes() == key + key and idx.tolist() == [1]
    assert mb.shape == (1, 3) and ml.tolist() == [3] and mb.tobytes() == b"abc"
    assert sb.shape == (1, 96) and sl.tolist() == [5] and sb.dtype == np.uint8  # padded to the scheme's width
    g2key = bytes([0x80]) + bytes(95)
    kb, key_len, idx, mb, ml, sb, sl = chain.pack_keyed(_lib.SCHEME_G1_RFC9380, [g2key], [0], [b""], [b""])
    assert (kb.size, key_len) == (96, 96) and sb.shape == (1, 48) and mb.shape[1] >= 1 and ml.tolist() == [0]
    for bad in (lambda: chain.pack_keyed(_lib.SCHEME_CHAINED, [], [], [], []),
                lambda: chain.pack_keyed(_lib.SCHEME_CHAINED, [g2key], [0], [b""], [b""]),
                lambda: chain.pack_keyed(_lib.SCHEME_CHAINED, [key], [1], [b""], [b""]),
                lambda: chain.pack_keyed(_lib.SCHEME_CHAINED, [key], [0, 0], [b""], [b""])):
        with pytest.raises(ValueError):
            bad()
    # an empty batch never needs a device
    assert chain.verify_keyed(chain.Scheme("pedersen-bls-chained", False), [key], [], [], []).size == 0


def test_identity_hash_and_wrong_length_keys_need_no_device():
    import hashlib
    from drand_amd import _lib, identity
    key = bytes(range(48))
    assert identity.identity_hash(key) == hashlib.blake2b(key, digest_size=32).digest()
    assert len(identity.identity_hash(key)) == 32
    assert identity.identity_reasons([(b"short", b"")]) == [_lib.REASON_KEY]
    assert identity.unsigned_identities([]) == []
