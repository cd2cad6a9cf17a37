"""Host check of the staging ring's copy pool (drand_amd/csrc/copy_pool.h):
every host record of dgpu_verify_beacons / dgpu_verify_recovered /
dgpu_verify_multi reaches the pinned ring through copy_pool::copy, split over
up to 8 threads.  tests/copy_pool_check.cpp (a stand-alone program, host code
only) sweeps the split of every size up to one ring slot -- parts in order,
disjoint, 64-byte-aligned starts, union exactly [0, bytes) -- copies
byte-exactly at the sizes where a split can lose its tail (4,194,564 bytes,
the sig_len array of 1,048,641 rounds, among them), and runs 8 concurrent
callers through one pool.  Built here under ASan + UBSan, and the concurrent
part again under TSan.  CPU test; each half is skipped only when a trivial
program cannot be built and started under its sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, sanitize):
    """The check program under -fsanitize=`sanitize`.  Skips only when a
    trivial program cannot be built and started with those flags (no
    sanitizer runtime here); a failure to build the real program fails."""
    flags = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
             "-fno-omit-frame-pointer"]
    probe_src = tmp / "probe.cpp"
    probe_src.write_text("#include <thread>\nint main() { std::thread([] {}).join(); }\n")
    p = subprocess.run(flags + ["-o", str(tmp / "probe"), str(probe_src)], capture_output=True, text=True)
    if p.returncode:
        pytest.skip(f"-fsanitize={sanitize} build unavailable: " + p.stderr[-300:])
    p = subprocess.run([str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode:  # e.g. TSan refusing the address-space layout
        pytest.skip(f"-fsanitize={sanitize} runtime unavailable: " + p.stderr[-300:])
    exe = tmp / name
    p = subprocess.run(flags + ["-I", os.path.join(ROOT, "drand_amd", "csrc"), "-o", str(exe),
                                os.path.join(ROOT, "tests", "copy_pool_check.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _run(exe, part, env):
    p = subprocess.run([exe, part], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


def test_copy_pool_split_and_copies_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "copy_pool_check", "address,undefined")
    out = _run(exe, "all", {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    # every size in [1, 16 MiB + 64]; 98 sizes x 5 alignments; 8 callers x 50 copies
    assert "copy_pool_check: split=16777280 copies=490 concurrent=400 failures=0 ok" in out, out


def test_copy_pool_concurrent_callers_under_tsan(tmp_path):
    exe = _build(tmp_path, "copy_pool_check_tsan", "thread")
    out = _run(exe, "concurrent", {"TSAN_OPTIONS": "halt_on_error=1"})
    assert "copy_pool_check: split=0 copies=0 concurrent=400 failures=0 ok" in out, out
