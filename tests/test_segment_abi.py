"""The two linked-segment entry points at the ABI: include/drand_gpu.h declares
them, drand_amd/_lib.py binds them with as many arguments as the header
lists, the library exports them, and the ABI version is still 3 (the change
is additive).  CPU-only."""
import os
import re

from conftest import ROOT
from test_abi import declared_params as _declared_params

NAMES = ("dgpu_verify_segment", "dgpu_verify_segment_device")


def test_header_declares_the_segment_entry_points():
    host = _declared_params("dgpu_verify_segment")
    dev = _declared_params("dgpu_verify_segment_device")
    assert len(host) == 16 and len(dev) == 17
    assert [p.split()[-1].lstrip("*") for p in host] == [
        "ctx", "scheme", "pk", "pk_len", "first_round", "n", "sigs", "sig_stride", "sig_len", "seed_prev",
        "seed_prev_len", "mode", "rlc_seed", "verdict_bits", "reason", "randomness32"]
    assert dev[-1].split()[-1].lstrip("*") == "stream" and dev[4].startswith("uint64_t")


def test_binding_matches_the_header():
    from drand_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NAMES:
        assert name in bound, name
        res, args = bound[name]
        assert res is _lib.ctypes.c_int
        assert len(args) == len(_declared_params(name)), name
        # first_round and rlc_seed are 64-bit values, n and the strides size_t
        assert args[4] is _lib.ctypes.c_uint64 and args[12] is _lib.ctypes.c_uint64
        assert args[5] is _lib.ctypes.c_size_t and args[7] is _lib.ctypes.c_size_t and args[10] is _lib.ctypes.c_size_t


def test_library_exports_them_and_abi_version_stays_3():
    from drand_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.dgpu_abi_version() == 3 == _lib.ABI_VERSION
    txt = open(os.path.join(ROOT, "include", "drand_gpu.h")).read()
    assert re.search(r"#define DGPU_ABI_VERSION 3\b", txt)
    # nothing of the feature went into the ingest header, whose symbol list is pinned
    assert "segment" not in open(os.path.join(ROOT, "include", "drand_ingest.h")).read()
