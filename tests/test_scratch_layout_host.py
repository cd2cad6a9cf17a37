"""Host check of the device scratch layouts (drand_amd/csrc/scratch_layouts.h:
one description per buffer gives its size and its regions).

tests/scratch_layout_check.hip is a stand-alone program, host code only, built
like tests/park_layout_check.hip (hipcc --cuda-host-only) plus ASan + UBSan;
it is not loaded into Python.  It fills the layout structs the library carves
its buffers with, over heap blocks of exactly the layouts' own byte counts, and
calls the index functions the kernels call.  For n = 1, 4, 5, 6 (the 5-round
engine block), 63, 64, 65 (the 64-round wave and park block) and 2, 3 (the
segment trees' smallest levels) it checks that every layout's regions are
ordered, disjoint, aligned and end at the byte count; that the byte count and
every region offset equal the recorded values of the expressions the layouts
replaced (n = 1 and n = 65); that the wave-blocked index functions stay inside
their regions for every round below n; and that the first and last element of
every region can be written: an access past the sizing is an ASan error.
CPU test; built without the sanitizers only when a trivial program cannot be
built and started under them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scratch_layout_check.hip")
LAYOUTS = 31         # buffers checked per run
RECORDED_FIXED = 12  # layouts without a round count: their recorded offsets are checked in every run
RECORDED_PER_N = 18  # ... and those with one, at n = 1 and n = 65


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scratch_layout_check")
    # -O0: the headers' field arithmetic comes along as out-of-line host functions (see test_park_layout_host.py)
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
    exe = tmp / "scratch_layout_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 63, 64, 65])
def test_scratch_layouts(check_exe, n):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([check_exe, str(n)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    recorded = RECORDED_FIXED + (RECORDED_PER_N if n in (1, 65) else 0)
    out = p.stdout
    assert f"scratch_layout_check: n={n} layouts={LAYOUTS} " in out and f" expected={recorded} failures=0 ok" in out, out
