"""ctypes binding of libdrand_gpu.so (the C-ABI in include/drand_gpu.h).

The product path has no CPU fallback: if the library is missing or no gfx950
GPU is available, opening a context raises DrandGPUError.
"""
import ctypes
import sys
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRAND_GPU_LIB selects an alternative in-tree build (A/B experiments only)
LIB_PATH = os.environ.get("DRAND_GPU_LIB") or os.path.join(_HERE, "libdrand_gpu.so")
# The same sources built with -DDG_AB_KNOBS (__graft_entry__.build): the only
# build that reads the A/B variant knobs and test hooks (AB_KNOBS) from the
# environment.  Tests open it for those variants; the product never loads it.
AB_LIB_PATH = os.path.join(_HERE, "libdrand_gpu_ab.so")
AB_KNOBS = frozenset({"DGPU_DEC_OVERLAP", "DGPU_MSM_SEG", "DGPU_LANE_SLICES", "DGPU_KB_NORM", "DGPU_RLC_DESCENT_STEP",
                      "DGPU_RLC_LOCALIZE", "DGPU_G1_LINES", "DGPU_SUBGROUP", "DGPU_RECOVER", "DGPU_RECOVER_ROWS",
                      "DGPU_RECOVER_WIDE_BUDGET",
                      "DGPU_KB_INV_CHAIN", "DGPU_KB_TEST_FLAG", "DGPU_TEST_ALLOC_CAP", "DGPU_STAGE",
                      "DGPU_ENG_XW", "DGPU_TEST_STAGE_ONLY", "DGPU_LINES_WAVE", "DGPU_KB_PAIR", "DGPU_TEST_FORCE_EXC",
                      "DGPU_REDUCE_NORM", "DGPU_KEYED_RANGE", "DGPU_TEST_MILLER_MARK",
                      "DGPU_TEST_FE_MARK"})

DGPU_OK = 0
DGPU_EINVAL = -1
DGPU_EDEVICE = -2
DGPU_ENOMEM = -3
DGPU_EUNSUPPORTED = -4
DGPU_ENOKEY = -5

SCHEME_CHAINED = 0
SCHEME_UNCHAINED = 1
SCHEME_UNCHAINED_G1 = 2
SCHEME_G1_RFC9380 = 3

MODE_PER_ROUND = 0
MODE_RLC = 1

REASON_OK = 0
REASON_DECODE = 1
REASON_SUBGROUP = 2
REASON_PAIRING = 3
REASON_INFINITY = 4
REASON_KEY = 5  # the record's key (dgpu_verify_keyed): rejected, or an index outside the table

# every symbol include/drand_gpu.h declares: (name, restype, argtypes)
_c = ctypes
_P = _c.c_void_p
SYMBOLS = [
    ("dgpu_abi_version", _c.c_int, []),
    ("dgpu_last_error", _c.c_char_p, []),
    ("dgpu_open", _c.c_int, [_c.c_int, _c.POINTER(_P)]),
    ("dgpu_close", None, [_P]),
    ("dgpu_scheme_from_name", _c.c_int, [_c.c_char_p]),
    ("dgpu_set_pubkey", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t]),
    ("dgpu_verify_batch", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t, _P,
                                     _c.c_int, _c.c_uint64, _P, _P]),
    ("dgpu_verify_batch_device", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t,
                                            _P, _c.c_int, _c.c_uint64, _P, _P, _P]),
    ("dgpu_set_profiling", _c.c_int, [_P, _c.c_int]),
    ("dgpu_staging_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_uint64)]),
    ("dgpu_synchronize", _c.c_int, [_P]),
    ("dgpu_stage_times", _c.c_int, [_P, _c.POINTER(_c.c_float), _c.c_int, _c.POINTER(_c.c_char_p)]),
    ("dgpu_digest_batch", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P]),
    ("dgpu_hash_to_g2", _c.c_int, [_P, _c.c_size_t, _P, _P]),
    ("dgpu_hash_to_g1", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _P]),
    ("dgpu_derive_pubkey", _c.c_int, [_P, _c.c_int, _P, _P, _c.c_size_t]),
    ("dgpu_make_chain", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P]),
    ("dgpu_set_group", _c.c_int, [_P, _c.c_int, _c.c_int, _P]),
    ("dgpu_set_group_scheme", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_size_t]),
    ("dgpu_set_group_wide", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_size_t]),
    ("dgpu_recover_batch_device", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _P, _P]),
    ("dgpu_make_partials", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _c.c_size_t, _P]),
    ("dgpu_make_partials_scheme", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _c.c_size_t,
                                             _P]),
    ("dgpu_recover_batch", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _P]),
    ("dgpu_shard_range", None, [_c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t)]),
    ("dgpu_verify_beacons", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P,
                                       _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P]),
    ("dgpu_verify_beacons_device", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _c.c_size_t, _P,
                                              _P, _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P, _P]),
    ("dgpu_decode_rows_device", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _P, _c.c_size_t, _P, _P,
                                           _c.c_size_t, _P, _P, _P]),
    ("dgpu_verify_rows", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _P, _c.c_size_t, _c.c_size_t,
                                    _c.c_int, _c.c_uint64, _P, _P, _P, _P]),
    ("dgpu_faulty_rounds_device", _c.c_int, [_P, _c.c_uint64, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P, _P, _P,
                                             _c.c_size_t, _P, _c.c_size_t, _P, _P]),
    ("dgpu_check_rows", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P, _c.c_size_t,
                                   _c.c_size_t, _c.c_int, _c.c_uint64, _c.c_uint64, _c.c_size_t, _P, _P, _c.c_size_t,
                                   _P, _P, _c.c_size_t, _P, _P]),
    ("dgpu_verify_segment", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P, _c.c_size_t, _P,
                                       _P, _c.c_size_t, _c.c_int, _c.c_uint64, _P, _P, _P]),
    ("dgpu_verify_segment_device", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P,
                                              _c.c_size_t, _P, _P, _c.c_size_t, _c.c_int, _c.c_uint64, _P, _P, _P,
                                              _P]),
    ("dgpu_verify_segment_shard_device", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P,
                                                    _c.c_size_t, _P, _P, _P, _c.c_int, _c.c_uint64, _P, _P, _P, _P]),
    ("dgpu_rlc_root_segment_device", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P,
                                                _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _c.c_uint64, _P, _P]),
    ("dgpu_rlc_root_bytes", _c.c_int, [_c.c_int]),
    ("dgpu_rlc_root_device", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P,
                                        _c.c_size_t, _P, _c.c_uint64, _P, _P]),
    ("dgpu_rlc_finish_device", _c.c_int, [_P, _c.c_size_t, _P, _P, _P, _P]),
    ("dgpu_verify_recovered", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _c.c_size_t, _P, _P,
                                         _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P]),
    ("dgpu_hash_to_curve", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _c.c_size_t, _P, _P]),
    ("dgpu_sign", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _P, _c.c_size_t, _P, _P]),
    ("dgpu_decode_g1_points", _c.c_int, [_P, _c.c_size_t, _P, _P, _P]),
    ("dgpu_decode_signatures", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P]),
    ("dgpu_decode_pubkey", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _P]),
    ("dgpu_multi_open", _c.c_int, [_c.c_int, _P, _c.POINTER(_P)]),
    ("dgpu_multi_close", None, [_P]),
    ("dgpu_multi_context", _c.c_int, [_P, _c.c_int, _c.POINTER(_P)]),
    ("dgpu_verify_multi", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P,
                                     _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P]),
    ("dgpu_verify_segment_multi", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P, _c.c_size_t,
                                             _P, _P, _c.c_size_t, _c.c_int, _c.c_uint64, _P, _P, _P]),
    ("dgpu_check_rows_multi", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P, _c.c_size_t,
                                         _c.c_size_t, _c.c_int, _c.c_uint64, _c.c_uint64, _c.c_size_t, _P, _P,
                                         _c.c_size_t, _P, _P, _c.c_size_t, _P, _P]),
    ("dgpu_multi_set_group", _c.c_int, [_P, _c.c_int, _c.c_int, _P]),
    ("dgpu_multi_set_group_scheme", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_size_t]),
    ("dgpu_multi_set_group_wide", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_size_t]),
    ("dgpu_recover_multi", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _P]),
    ("dgpu_verify_keyed", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _c.c_size_t, _c.c_size_t, _P, _P, _c.c_size_t, _P,
                                     _P, _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P]),
    ("dgpu_verify_keyed_device", _c.c_int, [_P, _c.c_int, _c.c_size_t, _P, _c.c_size_t, _c.c_size_t, _P, _P,
                                            _c.c_size_t, _P, _P, _c.c_size_t, _P, _c.c_int, _c.c_uint64, _P, _P, _P]),
    ("dgpu_verify_partials", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_int, _c.c_uint64,
                                        _P, _P]),
    ("dgpu_verify_partials_device", _c.c_int, [_P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_int,
                                               _c.c_uint64, _P, _P, _P]),
]

ABI_VERSION = 3


class DrandGPUError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"drand_gpu error {code}: {msg}")
        self.code = code


_libs = {}
_lib_lock = threading.Lock()


def load(path=None):
    """Load libdrand_gpu.so (or the build at `path`) once and bind every
    declared symbol (raises if absent)."""
    p = path or LIB_PATH
    with _lib_lock:
        if p in _libs:
            return _libs[p]
        if not os.path.exists(p):
            raise DrandGPUError(DGPU_EDEVICE, f"{p} not built (run __graft_entry__.build())")
        lib = ctypes.CDLL(p)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.dgpu_abi_version() != ABI_VERSION:
            raise DrandGPUError(DGPU_EINVAL, "ABI version mismatch")
        _libs[p] = lib
        return lib


def check(rc, lib=None):
    """Raise DrandGPUError for a failed call; the message is the failing
    library's thread-local dgpu_last_error (pass `lib` for a non-default build)."""
    if rc != DGPU_OK:
        lib = lib or load()
        raise DrandGPUError(rc, lib.dgpu_last_error().decode(errors="replace"))
    return rc


MAX_STAGES = 32  # DGPU_MAX_STAGES
NARROW_MAX_T = 32  # dgpu_set_group[_scheme]'s largest threshold; above it dgpu_set_group_wide
MAX_THRESHOLD = 1024  # DGPU_MAX_THRESHOLD
# recover_wide.cuh: window-table bytes per term by "signatures on G1", and one chunk's budget
# (tests/test_recover_wide_host.py compares all five with the headers' values)
RECW_TERM_BYTES = {False: 3136, True: 1792}
RECW_TABLE_BUDGET = 1 << 30


def stage_times(ctx):
    """dgpu_stage_times of the context's last profiled call: {stage: ms}.
    Raises on an overflowed event pool; every pipeline's stage count is
    within DGPU_MAX_STAGES (asserted: the return is the count needed)."""
    ms = (ctypes.c_float * MAX_STAGES)()
    names = (ctypes.c_char_p * MAX_STAGES)()
    ns = ctx.lib.dgpu_stage_times(ctx.handle, ms, MAX_STAGES, names)
    if ns < 0:
        check(ns, ctx.lib)
    if ns > MAX_STAGES:
        raise DrandGPUError(DGPU_EINVAL, f"{ns} stages > DGPU_MAX_STAGES")
    return {names[i].decode(): float(ms[i]) for i in range(ns)}


def staging_stats(ctx):
    """dgpu_staging_stats: (device_ms, host_ms, bytes) of the context's last
    host-record staging."""
    ms, hms, nb = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
    check(ctx.lib.dgpu_staging_stats(ctx.handle, ctypes.byref(ms), ctypes.byref(hms), ctypes.byref(nb)), ctx.lib)
    return ms.value, hms.value, nb.value


def shard_range(n, ndev, k):
    """dgpu_shard_range: item range [lo, hi) of device k (host-only bookkeeping)."""
    lib = load()
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    lib.dgpu_shard_range(n, ndev, k, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def ptr(buf):
    """Address of a numpy array / bytes-like / torch tensor for the C-ABI."""
    if buf is None:
        return None
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr()
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data
    raise TypeError(type(buf))


class Context:
    """One GPU context (dgpu_ctx*).  Thread-safe: the library serializes."""

    installed_group = None  # the key of the threshold group the context holds (calls.set_group)

    def __init__(self, device=0, lib_path=None):
        # torch bundles its own HIP runtime under the system one's SONAME: a
        # process that uses both must let torch initialise HIP first, or torch
        # later finds no GPU (Python callers)
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            torch.cuda.init()
        self.lib = load(lib_path)
        h = ctypes.c_void_p()
        check(self.lib.dgpu_open(device, ctypes.byref(h)), self.lib)
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self.lib.dgpu_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """dgpu_multi handle: one context per listed GPU and an RCCL communicator
    over them (dgpu_multi_open)."""

    def __init__(self, devices):
        self.lib = load()
        self.devices = list(devices)
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        check(self.lib.dgpu_multi_open(len(self.devices), arr, ctypes.byref(h)), self.lib)
        self.handle = h

    def close(self):
        if self.handle:
            self.lib.dgpu_multi_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
