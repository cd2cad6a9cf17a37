"""The index rule of the per-key sums (drand_amd/csrc/keyed_groups.h) and the
RLC scratch layout of the keyed calls, walked on the host.

tests/keyed_groups_check.cpp is a stand-alone program with its own main, host
code only: it is compiled here (with ASan + UBSan where a probe program
builds and starts with them) and run directly, never loaded into Python.
CPU-only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "keyed_groups_check.cpp")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("keyed_groups_check")
    # -O0: the layouts header brings the kernels' field arithmetic along as host functions; optimising them under the
    # sanitizers takes minutes (see test_scratch_layout_host.py)
    base = ["hipcc", "-O0", "-g", "-std=c++17", "--cuda-host-only", "-x", "hip"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = tmp / "probe.cpp"
    probe.write_text("#include <cstdlib>\nint main() { char* p = (char*)malloc(4); p[0] = 1; int r = p[0] - 1; free(p); return r; }\n")
    flags = base + san
    p = subprocess.run(flags + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode == 0:
        p = subprocess.run([str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode:  # no sanitizer runtime for this compiler here: the same program without it
        flags = base
    exe = tmp / "keyed_groups_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def test_rule_and_layout(check_exe):
    p = subprocess.run([check_exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "keyed_groups_check: cases=" in p.stdout and " failures=0 ok" in p.stdout, p.stdout
    assert int(p.stdout.split("cases=")[1].split()[0]) == 6 * 4 * 3 * 3 * 2, p.stdout


def test_check_program_detects_a_wrong_sum(check_exe):
    """The program compares: one changed expected sum is one failure."""
    p = subprocess.run([check_exe, "--perturb"], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 1 and "failures=1 FAILED" in p.stdout, (p.stdout, p.stderr[-2000:])
