"""The three entry points of linked segments across GPUs at the ABI:
include/drand_gpu.h declares dgpu_verify_segment_shard_device,
dgpu_rlc_root_segment_device and dgpu_verify_segment_multi with the documented
parameter names, drand_amd/_lib.py binds them with the same arity and the
64-bit / size_t types, the library exports them, and the ABI version is still
3 (the change is additive).  CPU-only."""
import os
import re

from conftest import ROOT
from test_abi import declared_params as _declared_params

PARAMS = {
    "dgpu_verify_segment_shard_device": [
        "ctx", "scheme", "pk", "pk_len", "first_round", "n", "d_sigs", "sig_stride", "d_sig_len", "d_halo",
        "d_halo_len", "mode", "rlc_seed", "d_verdict_bits", "d_reason", "d_randomness32", "stream"],
    "dgpu_rlc_root_segment_device": [
        "ctx", "scheme", "pk", "pk_len", "first_round", "n", "d_sigs", "sig_stride", "d_sig_len", "seed_prev",
        "seed_prev_len", "d_halo", "d_halo_len", "rlc_seed", "d_root", "stream"],
    "dgpu_verify_segment_multi": [
        "m", "scheme", "pk", "pk_len", "first_round", "n", "sigs", "sig_stride", "sig_len", "seed_prev",
        "seed_prev_len", "mode", "rlc_seed", "verdict_bits", "reason", "randomness32"],
}
# positions of the 64-bit values (first_round, rlc_seed) and of the size_t ones (pk_len, n, strides, lengths)
U64 = {"first_round", "rlc_seed"}
SIZE_T = {"pk_len", "n", "sig_stride", "seed_prev_len"}


def test_header_declares_the_entry_points():
    for name, want in PARAMS.items():
        got = _declared_params(name)
        assert [p.split()[-1].lstrip("*") for p in got] == want, name
        for p in got:
            pname = p.split()[-1].lstrip("*")
            if pname in U64:
                assert p.startswith("uint64_t "), (name, p)
            if pname in SIZE_T:
                assert p.startswith("size_t "), (name, p)
        # the halo is a device record and a device length
        if "d_halo" in want:
            assert "const uint8_t *d_halo" in got and "const uint32_t *d_halo_len" in got


def test_bindings_match_the_header():
    from drand_amd import _lib
    c = _lib.ctypes
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name, want in PARAMS.items():
        assert name in bound, name
        res, args = bound[name]
        assert res is c.c_int
        assert len(args) == len(want) == len(_declared_params(name)), name
        for pname, a in zip(want, args):
            if pname in U64:
                assert a is c.c_uint64, (name, pname)
            elif pname in SIZE_T:
                assert a is c.c_size_t, (name, pname)
            elif pname in ("scheme", "mode"):
                assert a is c.c_int, (name, pname)
            else:
                assert a is c.c_void_p, (name, pname)


def test_library_exports_them_and_abi_version_stays_3():
    from drand_amd import _lib
    lib = _lib.load()
    for name in PARAMS:
        assert hasattr(lib, name), name
    assert lib.dgpu_abi_version() == 3 == _lib.ABI_VERSION
    txt = open(os.path.join(ROOT, "include", "drand_gpu.h")).read()
    assert re.search(r"#define DGPU_ABI_VERSION 3\b", txt)


def test_python_surfaces_exist():
    """MultiVerifier.verify_segment has Verifier.verify_segment's signature
    (so sync.trusted_previous_signature_segments takes either), and dist has
    the sharded call and its halo exchange."""
    import inspect
    from drand_amd import chain, dist, multi
    one = inspect.signature(chain.Verifier.verify_segment)
    many = inspect.signature(multi.MultiVerifier.verify_segment)
    assert list(one.parameters) == list(many.parameters) == [
        "self", "first_round", "sigs", "prev_sig", "pubkey", "mode", "rlc_seed", "randomness", "sig_len"]
    assert [p.default for p in one.parameters.values()] == [p.default for p in many.parameters.values()]
    assert list(inspect.signature(dist.verify_segment_sharded).parameters) == [
        "ctx", "code", "pk", "first_round", "n_total", "d_sigs", "d_sig_len", "seed_prev", "mode", "seed", "d_bits",
        "stream", "world", "rank", "d_reason", "d_randomness", "sig_stride"]
    assert callable(dist.exchange_halo)
