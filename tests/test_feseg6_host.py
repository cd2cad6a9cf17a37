"""Host checks of the six-lane FE segments (feseg6.cuh): the same DG_FN
functions k_eng_fe_seg6 runs, with the lanes emulated over arrays.

tests/hostsim/feseg6.hip is built here as a shared library without
sanitizers; built with -DFS6_MAIN it is a stand-alone program for sanitizer
runs.  CPU tests."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "feseg6.hip")
LIB = os.path.join(ROOT, "tests", "hostsim", "libdrand_feseg6.so")

ST_OK, ST_SUBGROUP, ST_PAIRING = 0, 2, 3
CNT = 21  # three waves: five blocks, so the last wave's second half repeats the last block

# flagged items -> the 5-round blocks the fallback list must name
FLAGS = {"none": ([], []),
         "first_item_of_a_block": ([5], [1]),
         "last_item_of_a_block": ([14], [2]),
         "both_blocks_of_a_wave": ([1, 3, 8], [0, 1])}


@pytest.fixture(scope="module")
def fs6():
    csrc = os.path.join(ROOT, "drand_amd", "csrc")
    deps = [SRC, os.path.join(ROOT, "tests", "hostsim", "hostsim.hip")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "--cuda-host-only", "-fPIC", "-shared", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def test_ops_match_tower(fs6):
    """The product (and the next product on its outputs), the conjugated
    product, both Frobenius maps, the squaring and conj on 64 seeded operand
    pairs and on operands at the stored values' limb maxima: the tower's
    residues (fp12_mul, fp12_conj, fp12_frob1, fp12_frob2, fp12_sqr), every
    stored value within its documented bound."""
    first = ctypes.c_int(0)
    assert fs6.fs6_random(64, ctypes.c_uint64(20), ctypes.byref(first)) == 0, first.value
    assert fs6.fs6_edge() == 0


def _segment(fs6, seg, flagged, seed):
    ones = (ctypes.c_uint8 * CNT)(*[1 if i % 4 == 3 else 0 for i in range(CNT)])  # these items' R is 1
    flags = (ctypes.c_uint8 * CNT)(*[1 if i in flagged else 0 for i in range(CNT)])
    st0 = [ST_SUBGROUP if i % 7 == 2 else ST_OK for i in range(CNT)]
    status = (ctypes.c_uint8 * CNT)(*st0)
    fb = (ctypes.c_uint32 * (1 + (CNT + 4) // 5))()
    rc = fs6.fs6_segment(seg, CNT, ctypes.c_uint64(seed), ones, flags, status, fb)
    return rc, st0, list(status), list(fb)


@pytest.mark.parametrize("seg", [1, 2, 3, 4])
def test_segment_matches_12_lane_program(fs6, seg):
    """Segments 1..4 on seeded planes: planes M, T, T2 and R are the residues
    hostsim's emulation of the same ENG_PROG_FEK segment leaves, the other
    planes and rounds past cnt untouched; no verdict, no fallback entry."""
    rc, st0, st, fb = _segment(fs6, seg, [1, 8], 40 + seg)
    assert rc == 0
    assert st == st0 and fb[0] == 0


@pytest.mark.parametrize("pattern", sorted(FLAGS))
def test_last_segment_verdicts_and_fallback_list(fs6, pattern):
    """Segment 5: the same residues; ST_PAIRING exactly for the unflagged
    ST_OK items whose R is not 1 (every fourth item's is 1), and the fallback
    list names each block with a flagged item once."""
    flagged, blocks = FLAGS[pattern]
    rc, st0, st, fb = _segment(fs6, 5, flagged, 45)
    assert rc == 0
    want = [ST_PAIRING if (s == ST_OK and i % 4 != 3 and i not in flagged) else s for i, s in enumerate(st0)]
    assert st == want
    assert fb[0] == len(blocks) and sorted(fb[1:1 + fb[0]]) == blocks


@pytest.mark.parametrize("cnt", [1, 4, 5, 6, 9, 10, 11, 14, 15, 16, 63, 64, 65])
def test_addresses_inside_planes(fs6, cnt):
    """The largest word k_eng_fe_seg6 addresses in the state planes, over the
    five segments, lies inside the eng_kb_layout planes of eng_blocks(cnt)
    blocks, and its word pairs are 8-byte aligned."""
    out = (ctypes.c_uint64 * 3)()
    fs6.fs6_extents(ctypes.c_uint64(cnt), out)
    mx, words, odd = list(out)
    assert 0 < mx <= words and not odd
    assert words == ((cnt + 4) // 5) * 9 * 14 * 60
    if cnt % 5 == 0:  # whole blocks: the last item's last word is the last plane's last
        assert mx == words
