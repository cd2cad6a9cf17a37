"""Host checks of fp_reduce_lz (fp.cuh): the reduction taken straight from
lazy limbs against the carried form fp_reduce(fp_norm(x)) it replaces, in the
field, in kb_sqr_thr (kb_thread.cuh) and in the T-steps (lines_thread.cuh).

tests/hostsim/reduce_lazy.hip holds both forms (template parameter LZ) of the
same device functions, host code only.  It is built here as a shared library
without sanitizers; built with -DRL_MAIN it is a stand-alone program for
sanitizer runs.  CPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "reduce_lazy.hip")
LIB = os.path.join(ROOT, "tests", "hostsim", "libdrand_reduce_lazy.so")

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
BITS, LIMBS, MASK = 28, 14, (1 << 28) - 1
R = 1 << (BITS * LIMBS)
PTOP1 = (P >> (BITS * (LIMBS - 1))) + 1


@pytest.fixture(scope="module")
def rl():
    csrc = os.path.join(ROOT, "drand_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "--cuda-host-only", "-fPIC", "-shared", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def value(limbs):
    return sum(int(x) << (BITS * i) for i, x in enumerate(limbs))


def normalized(v):
    """v < 2^392 as 14 limbs < 2^28."""
    return [(v >> (BITS * i)) & MASK for i in range(LIMBS)]


def lazy(v, lend):
    """The same value with `lend` units of each limb above the lowest moved
    down into the limb below (limbs up to 2^28 (lend + 1)): an unnormalized
    representation as the lazy sums produce."""
    l = normalized(v)
    for i in range(LIMBS - 1, 0, -1):
        t = min(lend, l[i])
        l[i] -= t
        l[i - 1] += t << BITS
    assert all(0 <= x < 1 << 32 for x in l) and value(l) == v
    return l


def run_reduce(rl, vecs):
    x = np.ascontiguousarray(np.array(vecs, dtype=np.uint32))
    n = len(x)
    outs = [np.zeros((n, LIMBS), dtype=np.uint32) for _ in range(4)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = rl.rl_reduce(p(x), n, *[p(o) for o in outs])
    return bad, outs


def check_reduce(rl, vecs):
    """residues equal the carried form's and the integer's own; output CI."""
    bad, (lz, ref, canon_lz, canon_ref) = run_reduce(rl, vecs)
    assert bad == 0
    assert np.array_equal(canon_lz, canon_ref)
    assert int(lz.max()) <= MASK
    rinv = pow(R, -1, P)
    for v, out, can in zip(vecs, lz, canon_lz):
        ov = value(out)
        assert ov < 2.01 * P and ov % P == value(v) % P      # CI, same residue as the input
        assert value(can) == value(v) * rinv % P             # the canonical (non-Montgomery) residue


def test_reduce_lz_random(rl):
    rng = np.random.default_rng(20261020)
    x = rng.integers(0, 1 << 32, size=(110000, LIMBS), dtype=np.uint64)
    # value < 2^392: the top limb and the carries into it stay below 2^28
    x[:, LIMBS - 1] &= MASK
    keep = [i for i in range(len(x)) if value(x[i]) < R][:100000]
    assert len(keep) == 100000
    x = x[keep].astype(np.uint32)
    bad, (lz, ref, canon_lz, canon_ref) = run_reduce(rl, x)
    assert bad == 0
    assert np.array_equal(canon_lz, canon_ref)
    assert int(lz.max()) <= MASK
    assert int(lz[:, LIMBS - 1].max()) < 214091              # < 2.01p
    rinv = pow(R, -1, P)
    for i in range(0, len(x), 97):                            # a sample against the integers
        assert value(lz[i]) % P == value(x[i]) % P
        assert value(canon_lz[i]) == value(x[i]) * rinv % P


def test_reduce_lz_edges(rl):
    full = (1 << 32) - 1
    low = [full] * (LIMBS - 1)
    carry = value(low + [0]) >> (BITS * (LIMBS - 1))          # what the low limbs carry into the top one: 16
    vecs = []
    vecs.append(low + [(1 << BITS) - 1 - carry])              # the largest admissible top limb
    assert value(vecs[-1]) < R <= value(low + [(1 << BITS) - carry])
    for k in (1, 2, 1000, (1 << BITS) // PTOP1 - 1):          # top limb a multiple of PTOP1, less what the low limbs
        for d in range(0, carry + 2):                         # carry: the carried form's quotient is one more
            vecs.append(low + [k * PTOP1 - d])
            vecs.append([MASK] * (LIMBS - 1) + [k * PTOP1 - d])
    for v in (0, P, 2 * P, P - 1, P + 1, 2 * P - 1, 2 * P + 1):
        vecs.append(normalized(v))
        if v:
            vecs.append(lazy(v, 7))
    # the documented maxima of the replaced sites (kb_t_out: 65.3p, 103.4p, 133p, 203p; the T-step: 33.2p)
    # and fp_add / fp_sub / fp2_sub32 / t2 (4.02p, 10.01p, 34.1p, 120.2p), normalized and lazy
    for m in (65.3, 103.4, 133, 203, 33.2, 4.02, 10.01, 34.1, 120.2):
        v = int(m * 1000) * P // 1000
        for w in (v, v - 1, v - P // 3):
            vecs.append(normalized(w))
            vecs.append(lazy(w, 3))
            vecs.append(lazy(w, 7))
            vecs.append(lazy(w, 15))
    check_reduce(rl, vecs)


def _golden_args():
    g = load_golden("chain_chained_s1.json")
    r = g["rounds"][0]
    prev = bytes.fromhex(r["prev"])
    return bytes.fromhex(g["pk"]), prev, len(prev), ctypes.c_uint64(r["round"]), bytes.fromhex(r["sig"])


def test_kb_sqr_thr_forms_agree(rl):
    """63 squarings from 64 seeded cyclotomic elements and from the five chain
    inputs of the golden pairing: both forms' four coordinates are the same
    residues (and fp12_cyclo_sqr's) and CI after every squaring."""
    first = ctypes.c_int(0)
    assert rl.rl_kb_random(64, ctypes.c_uint64(15), ctypes.byref(first)) == 0, first.value
    assert rl.rl_kb_golden(*_golden_args(), ctypes.byref(first)) == 0, first.value
    assert rl.rl_kb_edge() == 0                               # the largest CI start: limbs nearest 2^32


def test_lt_steps_forms_agree(rl):
    """The 68 T-steps of the golden (pk, H) and (-g1, sigma) pairs: every
    emitted coefficient and the final T are the same residues in both forms."""
    assert rl.rl_lines_golden(*_golden_args()) == 0
