"""Host checks of the six-lane Miller arithmetic (miller6.cuh): the same
DG_FN functions k_eng_miller6 runs, with the lanes emulated over arrays.

tests/hostsim/miller6.hip is built here as a shared library without
sanitizers; built with -DM6_MAIN it is a stand-alone program for sanitizer
runs.  Also the CPU check of the GPU test's corruption maps
(miller6_cases.py).  CPU tests."""
import ctypes
import os
import subprocess

import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "miller6.hip")
LIB = os.path.join(ROOT, "tests", "hostsim", "libdrand_miller6.so")


@pytest.fixture(scope="module")
def m6():
    csrc = os.path.join(ROOT, "drand_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "--cuda-host-only", "-fPIC", "-shared", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def test_products_and_squaring_match_tower(m6):
    """Three doubling steps (squaring, two line products) from 64 seeded
    starts, and one from operands at the stored values' limb maxima: every
    coefficient and its xi-form are the tower's residues (fp12_sqr,
    fp12_mul_line), every stored value within its documented bound."""
    first = ctypes.c_int(0)
    assert m6.m6_random(64, ctypes.c_uint64(19), 3, ctypes.byref(first)) == 0, first.value
    assert m6.m6_edge() == 0


@pytest.mark.parametrize("cnt", [1, 11])
def test_full_loop_on_golden_lines(m6, cnt):
    """The whole loop over the golden (pk, H), (-g1, sigma) lines, through the
    kernel's own addressing (11 items: two waves, an odd number of blocks):
    f is the tower's product of the same lines, as slot values."""
    g = load_golden("chain_chained_s1.json")
    r = g["rounds"][0]
    prev = bytes.fromhex(r["prev"])
    assert m6.m6_golden(bytes.fromhex(g["pk"]), prev, len(prev), ctypes.c_uint64(r["round"]), bytes.fromhex(r["sig"]),
                        cnt) == 0


@pytest.mark.parametrize("cnt", [1, 4, 5, 6, 9, 10, 11, 14, 15, 16, 63, 64, 65])
def test_addresses_inside_buffers(m6, cnt):
    """The largest word k_eng_miller6 addresses in the line and f buffers lies
    inside eng_blk_words(eng_blocks(cnt), .), and its word pairs are 8-byte
    aligned."""
    out = (ctypes.c_uint64 * 5)()
    m6.m6_extents(ctypes.c_uint64(cnt), out)
    max_l, max_f, lw, fw, odd = list(out)
    assert 0 < max_l <= lw and 0 < max_f <= fw and not odd
    if cnt % 5 == 0:  # whole blocks: the last item's last word is the line buffer's last; f fills plane 0 of 2
        assert max_l == lw and max_f == fw - 14 * 60


def test_gpu_cases_have_valid_and_corrupted_rounds():
    """The corruption maps of tests/test_gpu_miller6.py, from the seeds alone:
    every size of two rounds and more keeps valid rounds beside corrupted
    ones, so neither an all-pass nor an all-fail kernel can pass; the single
    round runs both clean and corrupted."""
    import numpy as np
    from drand_amd import _lib
    from drand_amd.synth import Chain, corrupt
    from miller6_cases import CASES, RATE, SIZES, corrupt_seed, kinds_for
    assert SIZES == [1, 5, 6, 10, 11, 21, 64, 65]
    for n in SIZES:
        # synth.corrupt itself, as the GPU test calls it, on a chain of the same shape (its map depends on the
        # seed, the length and the kinds alone)
        dummy = Chain(_lib.SCHEME_CHAINED, b"", np.arange(1, n + 1, dtype=np.uint64), np.ones((n, 96), dtype=np.uint8),
                      np.full(n, 96, dtype=np.uint32), np.ones((n, 96), dtype=np.uint8), np.full(n, 96, dtype=np.uint32),
                      b"")
        bad = corrupt(dummy, corrupt_seed(n), rate=RATE, kinds=kinds_for(n))
        assert len(bad) >= 1 and set(bad.values()) <= set(kinds_for(n))
        if n >= 2:
            assert len(bad) < n, n
    assert (1, True) in CASES and (1, False) in CASES
