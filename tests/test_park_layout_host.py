"""Host check of k_h2c_finish's park region (kernels.cuh h2c_park_word,
h2c_park_words, h2c_finish_stash).

tests/park_layout_check.hip is a stand-alone program, host code only, built
like tests/segment_src_check.hip (hipcc --cuda-host-only) plus ASan + UBSan;
it is not loaded into Python.  It includes the offset helper and the stash
the kernel uses -- they are host and device functions -- and for n = 1, 63,
64, 65 and 257 rounds (one round, a block less one, a whole block, a block
and one, four blocks and one) checks that the offsets of all (round, slot,
word) are distinct, lie below the sizing expression and are 16-byte aligned
per quad, and that random points put into every slot of every round come back
exactly.  The region is a heap allocation of exactly the sizing expression:
an access past it is an ASan error, a misaligned 16-byte access a UBSan error.
CPU test; built without the sanitizers only when a trivial program cannot be
built and started under them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "park_layout_check.hip")
SLOTS, WORDS = 3, 84


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("park_layout_check")
    # -O0: the header's field arithmetic comes along as out-of-line host functions, and
    # instrumenting it optimised takes the compiler tens of minutes; unoptimised, under a minute
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
    exe = tmp / "park_layout_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_park_offsets_and_round_trip(check_exe, n):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([check_exe, str(n), str(9000 + n)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    words = (n + 63) // 64 * 64 * SLOTS * WORDS  # whole blocks: 1008 bytes per round of ceil(n / 64) * 64
    assert (f"park_layout_check: n={n} words={words} offsets={n * SLOTS * WORDS} points={n * SLOTS} "
            "failures=0 ok") in p.stdout, p.stdout
