"""Host check of the check-chain rule (drand_amd/csrc/check_rows.cuh:
check_rows_slot, check_rows_outcome) and of the faulty list's scratch layout
(scratch_layouts.h: check_rows_layout, check_lists_layout; ingest_rows_layout
beside them).

tests/check_rows_check.cpp is a stand-alone program with its own main, host
code only: the headers under DG_NO_KERNELS, compiled as HIP host code (the
layouts header takes the other kernels' sizes from their headers, which need
the HIP runtime's types) with ASan + UBSan where a probe program builds and
starts under them, as tests/test_scratch_layout_host.py builds its program.
It is run directly, never loaded into Python.  It compares the rule with a
naive restatement of the loop at chain/beacon/sync_manager.go:188-222 over
hand-made and random windows, walks the four kernels' index arithmetic over a
heap block of exactly the layout's byte count (counts 1, 63, 64, 65, 255,
256, 257, 513 and 65,537 -- one above a single pass of the block-sum scan),
and checks the layouts' regions.  CPU test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "check_rows_check.cpp")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("check_rows_check")
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
    exe = tmp / "check_rows_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def test_rule_and_layout(check_exe):
    p = subprocess.run([check_exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "check_rows_check: cases=" in p.stdout and " failures=0 ok" in p.stdout, p.stdout
    cases = int(p.stdout.split("cases=")[1].split()[0])
    layouts = int(p.stdout.split("layouts=")[1].split()[0])
    assert cases >= 60 and layouts == 9 * (1 + 2 + 4), p.stdout


def test_check_program_detects_a_wrong_value(check_exe):
    """The program compares: one changed expected value is one failure."""
    p = subprocess.run([check_exe, "--perturb"], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 1 and "failures=1 FAILED" in p.stdout, (p.stdout, p.stderr[-2000:])
