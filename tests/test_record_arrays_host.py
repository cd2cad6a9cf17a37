"""Host check of the one description of a call's record arrays
(drand_amd/csrc/record_arrays.h), which the library's staging functions loop
over: the device buffers and rewritten pointers (stage_prepare_locked), the
copies through the ring in their order (host_stager::stage_slice), the pageable
copy (stage_inputs_locked), the length checks and the staged-byte count that
dgpu_staging_stats reports.

tests/record_arrays_check.hip is a stand-alone program with its own main, host
code only, built like tests/halo_src_check.hip (hipcc -O0 --cuda-host-only)
plus ASan + UBSan where a probe program builds and starts under them.  It
builds a 17-item call of each source kind with the library's own builders and
compares record_arrays' list with the expectations written here: the entries
and their order (once-per-call entries, message part, signature part), bytes
per item, the pad byte, the length array each is checked against, and the
staged bytes per item -- the figures the project documents and its GPU tests
assert: 208 per round for explicit chained records at strides 96/96,
sig_stride + 4 = 100 for the linked forms, msg_stride + 4 + sig_stride + 4 for
raw messages; the halo record and its length count 0, so the chained halo form
stages the linked form's 100.  The length checks run over the slices [0, 8) and
[8, 17): a bad length fails only the slice that holds it, with its global
index in the message.  CPU test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "record_arrays_check.hip")

SIGS = [("sigs", "sig", None, 0, "-"), ("sig_len", "sig", 4, 0, "-")]  # (None: the signature stride)


def _list_line(kind, chained, sig_stride, stride2, bytes_per_item, entries):
    """entries: (name, part, item_bytes, pad, len_name)."""
    out = [f"list {kind} {int(chained)} {sig_stride} {stride2} {bytes_per_item} {len(entries)}"]
    out += [f"  {nm} {part} {sig_stride if b is None else b} {pad} {ln}" for nm, part, b, pad, ln in entries]
    return "\n".join(out)


def _cases():
    records = [("rounds", "msg", 8, 0, "-"), ("prev", "msg", 96, 1, "prev_len"), ("prev_len", "msg", 4, 0, "-")]
    halo = [("halo", "once", None, 0, "-"), ("halo_len", "once", 4, 0, "-")]

    def raw(ms):
        return [("msgs", "msg", ms, 1, "msg_len"), ("msg_len", "msg", 4, 0, "-")]
    return [
        # explicit records: 8 + (96 + 4) + (96 + 4) = 208 per chained round; rounds and signatures alone unchained
        _list_line("records", True, 96, 96, 208, records + SIGS),
        _list_line("records", False, 96, 96, 8 + 96 + 4, records[:1] + SIGS),
        _list_line("records", False, 48, 0, 8 + 48 + 4, records[:1] + SIGS),
        # raw messages: msg_stride + 4 + sig_stride + 4
        _list_line("raw", False, 96, 32, 32 + 4 + 96 + 4, raw(32) + SIGS),
        _list_line("raw", False, 48, 40, 40 + 4 + 48 + 4, raw(40) + SIGS),
        # the linked seed form: the signature arrays alone, sig_stride + 4
        _list_line("linked", True, 96, 0, 100, SIGS),
        _list_line("linked", False, 96, 0, 100, SIGS),
        _list_line("linked", False, 48, 0, 52, SIGS),
        # the halo form: its one record and length once per call, 0 staged bytes
        _list_line("halo", True, 96, 0, 100, halo + SIGS),
        _list_line("halo", False, 96, 0, 100, SIGS),
    ]


def _bad_line(kind, item, slice_k):
    name = "msg" if kind == "raw" else "prev"
    return f"bad {kind} {item} 97 {slice_k} {name}_len[{item}]=97~>~{name}_stride"


BAD = [_bad_line("records", 7, 0), _bad_line("records", 8, 1), _bad_line("raw", 16, 1)]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_arrays_check")
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
    exe = tmp / "record_arrays_check"
    p = subprocess.run(flags + ["-o", str(exe), SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _run(exe, tmp_path, lines):
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, str(case)], capture_output=True, text=True, env=env, timeout=120)


def test_record_arrays_of_every_source_kind(check_exe, tmp_path):
    lists = _cases()
    p = _run(check_exe, tmp_path, lists + BAD)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert f"record_arrays_check: lists={len(lists)} bad_lengths={len(BAD)} failures=0 ok" in p.stdout, p.stdout


def test_check_program_detects_wrong_expectations(check_exe, tmp_path):
    """The program compares: a wrong byte count, a swapped order and a bad
    length expected in the other slice are one failure or more each."""
    wrong_bytes = _cases()[0].replace(" 208 ", " 204 ")
    p = _run(check_exe, tmp_path, [wrong_bytes])
    assert p.returncode == 1 and "208 staged bytes per item, want 204" in p.stderr, (p.stdout, p.stderr[-2000:])
    swapped = _list_line("linked", True, 96, 0, 100, SIGS[::-1])
    p = _run(check_exe, tmp_path, [swapped])
    assert p.returncode == 1 and "entry 0: not the field sig_len" in p.stderr, (p.stdout, p.stderr[-2000:])
    p = _run(check_exe, tmp_path, [_bad_line("records", 8, 0)])
    assert p.returncode == 1 and "slice 0 passes" in p.stderr and "slice 1 fails (item 8)" in p.stderr, (p.stdout, p.stderr[-2000:])
