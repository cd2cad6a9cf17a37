"""Host check of the device row parser (drand_amd/csrc/ingest_row.cuh) against
dgpu_ingest_decode (drand_amd/csrc/ingest.cpp), the decoder it restates.

tests/ingest_rows_check.cpp is a stand-alone program with its own main: the
header under DG_NO_KERNELS with DG_FN a plain inline function, ingest.cpp
linked in as the oracle, built like tests/halo_src_check.hip's program with
ASan + UBSan where a probe program builds and starts under them.  Every row
lives in a heap block of exactly its length and every record in one of
exactly its stride; ok, round, both lengths and every byte of both strides
are compared, for the two-buffer form and for the in-place form the kernel
parses LDS with.  The corpus is tests/ingest_rows_corpus.py's.  The same
program checks copy_pool::gather, which stages those rows.  CPU test."""
import os
import subprocess

import pytest

from ingest_rows_corpus import corpus, marshal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ingest_rows_check.cpp")
ORACLE = os.path.join(ROOT, "drand_amd", "csrc", "ingest.cpp")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ingest_rows_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-DDG_NO_KERNELS", "-DDG_FN=inline"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = tmp / "probe.cpp"
    probe.write_text("#include <cstdlib>\nint main() { char* p = (char*)malloc(4); p[0] = 1; int r = p[0] - 1; free(p); return r; }\n")
    flags = base + san
    p = subprocess.run(flags + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode == 0:
        p = subprocess.run([str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode:  # no sanitizer runtime for this compiler here: the same program without it
        flags = base
    exe = tmp / "ingest_rows_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC, ORACLE], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _case(path, rows, sig_stride, prev_stride):
    path.write_text("".join(f"{sig_stride} {prev_stride} {r.hex() or '-'}\n" for _, r in rows))


@pytest.mark.parametrize("strides", [(96, 96), (48, 96)])
def test_parser_equals_the_host_decoder(check_exe, tmp_path, strides):
    rows = corpus(*strides)
    case = tmp_path / "case.txt"
    _case(case, rows, *strides)
    p = subprocess.run([check_exe, str(case)], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert f"ingest_rows_check: rows={len(rows)} " in p.stdout and "failures=0 ok" in p.stdout, p.stdout
    # the corpus is not all of one kind: the named canonical rows decode, the named others do not
    canonical = int(p.stdout.split("canonical=")[1].split()[0])
    assert 10 <= canonical < len(rows) // 2, p.stdout


def test_check_program_detects_a_wrong_record(check_exe, tmp_path):
    """The program compares: one flipped bit of one record is one failure."""
    case = tmp_path / "case.txt"
    _case(case, [("chained", marshal(b"\x01" * 96, 5, b"\x02" * 96))], 96, 96)
    p = subprocess.run([check_exe, str(case), "--perturb"], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == 1 and "failures=1 FAILED" in p.stdout, (p.stdout, p.stderr[-2000:])


def test_copy_pool_gather_under_asan_ubsan(check_exe):
    """copy_pool::gather against a serial gather: several threads, one
    thread, one row, rows listed with no bytes, and a run that starts inside
    the packed positions; the destination is a heap block of exactly the
    packed size."""
    p = subprocess.run([check_exe, "--gather"], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == 0 and "gather failures=0 ok" in p.stdout, (p.stdout, p.stderr[-3000:])
