"""Host check of the wide recovery path's host-callable parts
(drand_amd/csrc/recover_wide.cuh, the wide layouts of scratch_layouts.h).

tests/recover_wide_check.hip is a stand-alone program, host code only, built
like tests/scratch_layout_check.hip (hipcc --cuda-host-only) plus ASan +
UBSan; it is not loaded into Python.  It runs the one-inversion Lagrange steps
of k_recover_lagrange_wide thread by thread -- the kernel calls the same
functions from the same header -- and compares every coefficient's eight words
with fr_lagrange_at_zero (t = 1, 2, 33, 65, 1024; index sets random, ascending,
descending, with 0 and 65535, and the dense 1..t); carves the two wide layouts
over heap blocks of exactly their byte counts (regions ordered, disjoint,
aligned, first and last element of every row written at stride t); and walks
the chunk sizing (every round covered once, the tables under the budget, one
round per chunk and never zero when a round alone exceeds it).  CPU test;
built without the sanitizers only when a trivial program cannot be built and
started under them.  (At t = 1024 the serial form is compared on a spread
sample of the points: it costs an inversion per point.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "recover_wide_check.hip")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recover_wide_check")
    base = ["hipcc", "-O0", "-g", "-std=c++17", "--cuda-host-only"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = tmp / "probe.hip"
    probe.write_text("#include <cstdlib>\nint main() { char* p = (char*)malloc(4); p[0] = 1; int r = p[0] - 1; free(p); return r; }\n")
    flags = base + san
    p = subprocess.run(flags + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode == 0:
        p = subprocess.run([str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode:  # no sanitizer runtime for this compiler here: the same program without it
        flags = base
    exe = tmp / "recover_wide_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("t", [1, 2, 33, 65, 1024])
def test_wide_lagrange_equals_fr_lagrange_at_zero(check_exe, t):
    out = _run(check_exe, "lagrange", str(t))
    assert f"recover_wide_check: lagrange t={t} " in out and " failures=0 ok" in out, out


def test_wide_layouts(check_exe):
    out = _run(check_exe, "layouts")
    assert "recover_wide_check: layouts " in out and " failures=0 ok" in out, out


def test_wide_chunk_sizing(check_exe):
    out = _run(check_exe, "chunks")
    assert "recover_wide_check: chunks " in out and " failures=0 ok" in out, out


def test_python_constants_equal_the_headers(check_exe):
    """drand_amd/_lib.py restates RECOVER_MAX_T, DGPU_MAX_THRESHOLD, the window
    tables' bytes per term and their budget; the program prints the headers'."""
    import re
    import sys
    sys.path.insert(0, ROOT)
    from drand_amd import _lib
    out = _run(check_exe, "consts")
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out)}
    assert got == {"narrow_max_t": _lib.NARROW_MAX_T, "max_threshold": _lib.MAX_THRESHOLD,
                   "term_g2": _lib.RECW_TERM_BYTES[False], "term_g1": _lib.RECW_TERM_BYTES[True],
                   "budget": _lib.RECW_TABLE_BUDGET}
    txt = open(os.path.join(ROOT, "include", "drand_gpu.h")).read()
    assert int(re.search(r"#define DGPU_MAX_THRESHOLD (\d+)", txt).group(1)) == _lib.MAX_THRESHOLD
