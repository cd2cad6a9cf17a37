"""Host check of the halo message source (kernels.cuh msg_src_halo: one shard
of a linked segment, dgpu_verify_segment_shard_device).

tests/halo_src_check.hip is a stand-alone program with its own main, host code
only, built like tests/segment_src_check.hip (hipcc -O0 --cuda-host-only) plus
ASan + UBSan where a probe program builds and starts under them.  It calls the
helpers the kernels call -- msg_digest, msg_bad_record, msg_round are host and
device functions -- on a 17-record signature array (lengths 96, 0, 48, 95 and
one above the stride among them) under the slice offsets g0 = 0, 1, 5, 16 and
the halo lengths 0, 32, 48, 96 and stride + 4, and compares every digest with
the explicit msg_src on the shifted records and with hashlib's SHA-256 of
prev || BE64(round), computed here.  The halo is a heap buffer of exactly
min(len, stride) bytes, the arrays allocations of their exact size: a read
past the halo or past a record's stride is an ASan error.  The unchained pass
hands the source NULL halo pointers.  CPU test."""
import hashlib
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "halo_src_check.hip")
STRIDE, N = 96, 17
OVERLONG = 9  # the record whose sig_len exceeds the stride
LENGTHS = {0: 96, 1: 0, 2: 48, 3: 95, OVERLONG: STRIDE + 4, 15: 1, 16: 96}
OFFSETS = (0, 1, 5, 16)
FIRST_ROUND = (1 << 40) + 12345  # the high round bytes are not zero


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("halo_src_check")
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
    exe = tmp / "halo_src_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _records(rng):
    """17 records of exactly STRIDE bytes (every byte random, so bytes past a
    record's length would change a digest that read them) and their lengths."""
    recs = [bytes(rng.randrange(256) for _ in range(STRIDE)) for _ in range(N)]
    lens = [LENGTHS.get(g, 96) for g in range(N)]
    return recs, lens


def _case_text(halo, halo_len, recs, lens):
    """halo: the min(halo_len, STRIDE) bytes the halo buffer holds."""
    assert len(halo) == min(halo_len, STRIDE)

    def prev_of(g):
        return halo if g == 0 else recs[g - 1][:min(lens[g - 1], STRIDE)]
    lines = [f"{STRIDE} {N} {FIRST_ROUND}", f"{halo_len} {halo.hex() or '-'}",
             f"{len(OFFSETS)} " + " ".join(map(str, OFFSETS))]
    lines += [f"{ln} {r.hex()}" for r, ln in zip(recs, lens)]
    lines += [hashlib.sha256(prev_of(g) + struct.pack(">Q", FIRST_ROUND + g)).hexdigest() for g in range(N)]
    lines += [hashlib.sha256(struct.pack(">Q", FIRST_ROUND + g)).hexdigest() for g in range(N)]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("halo_len", [0, 32, 48, 96, STRIDE + 4])
def test_halo_source_digests_and_bad_records(check_exe, tmp_path, halo_len):
    rng = random.Random(2000 + halo_len)
    halo = bytes(rng.randrange(256) for _ in range(min(halo_len, STRIDE)))
    recs, lens = _records(rng)
    case = tmp_path / "case.txt"
    case.write_text(_case_text(halo, halo_len, recs, lens))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([check_exe, str(case)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    # items per pass: sum over g0 of (17 - g0); chained and unchained passes.  Bad
    # records, chained pass only: the item after the over-long record, seen by
    # the offsets <= it, and item 0 under the over-long halo, seen by g0 = 0.
    items = sum(N - g0 for g0 in OFFSETS)
    bad_halo = 1 if halo_len > STRIDE else 0
    seen = sum(1 for g0 in OFFSETS if g0 <= OVERLONG + 1) + bad_halo
    want = f"halo_src_check: digests={2 * items} bad_records={seen} bad_halo={bad_halo} failures=0 ok"
    assert want in p.stdout, p.stdout


def test_check_program_detects_a_wrong_digest(check_exe, tmp_path):
    """The program compares: one flipped expected digest is one failure."""
    rng = random.Random(7)
    recs, lens = _records(rng)
    text = _case_text(b"h" * 32, 32, recs, lens).split("\n")
    row = 3 + N  # expected chained digest of global item 0, the halo's
    text[row] = ("0" if text[row][0] != "0" else "1") + text[row][1:]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(text))
    p = subprocess.run([check_exe, str(case)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "g=0: halo digest != expected" in p.stderr, (p.stdout, p.stderr[-2000:])
