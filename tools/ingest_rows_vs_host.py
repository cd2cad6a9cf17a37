#!/usr/bin/env python3
"""Check-chain ingest with the rows decoded on the host against on the GPU.

One process, one GPU: a chained chain of --rounds rounds (a handful of them
corrupted) is written as a bolt beacon store, then CheckPastBeacons runs over
it with decode="host" and decode="device" alternated, --reps times each, in
per-round mode and in RLC mode, at windows of --window rounds.  Reported per
run: rounds/s and the process's CPU seconds per million rows
(resource.getrusage(RUSAGE_SELF): user + system, every thread), the quantity
device decoding exists to lower.  Every run's faulty list must equal the
construction's.

Then k_ingest_rows alone (dgpu_decode_rows_device on one window's packed
rows, device events around --kernel-reps launches): rows/s and the bytes it
moves per second (rows, positions and lengths read; records, lengths, rounds
and flags written), beside a plain device-to-device copy that moves the same
number of bytes (half read, half written); both rotate over buffer sets that
together exceed the last-level cache.  Between the two, the host's own work
per window with nothing on the GPU: the scan alone, and the scan with the
native host decode.

Prints plain text; profiles/r12/ingest_rows_vs_host.txt is one run's output.
"""
import argparse
import os
import resource
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hex_rows(a, lens):
    table = np.frombuffer(b"".join(b"%02x" % v for v in range(256)), dtype=np.uint8).reshape(256, 2)
    hx = table[a].reshape(a.shape[0], -1)
    return [bytes(hx[i, :2 * int(lens[i])]) for i in range(a.shape[0])]


def marshal_chain(c):
    sig_hex, prev_hex = hex_rows(c.sigs, c.sig_len), hex_rows(c.prev, c.prev_len)
    rows = []
    for i in range(len(c.rounds)):
        p = b'"' + prev_hex[i] + b'"' if c.prev_len[i] else b"null"
        rows.append(b'{"PreviousSig":' + p + b',"Round":' + str(int(c.rounds[i])).encode() + b',"Signature":"' +
                    sig_hex[i] + b'"}')
    return rows


def cpu_seconds():
    u = resource.getrusage(resource.RUSAGE_SELF)
    return u.ru_utime + u.ru_stime


SETS = 8  # buffer sets a timing rotates over: together far beyond the 256 MB last-level cache


def kernel_alone(ctx, rows, reps):
    import torch
    from drand_amd import calls
    n = len(rows)
    ln = np.array([len(r) for r in rows], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(ln, dtype=np.uint64)[:-1]]).astype(np.uint64)
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    sizes = (("rounds", 8 * n), ("sigs", 96 * n), ("sig_len", 4 * n), ("prev", 96 * n), ("prev_len", 4 * n), ("ok", n))
    moved = buf.size + 12 * n + sum(size for _, size in sizes)
    sets = []
    for _ in range(SETS):
        t = {"rows": torch.from_numpy(buf.copy()).cuda(), "off": torch.from_numpy(off.view(np.int64)).cuda(),
             "len": torch.from_numpy(ln.view(np.int32)).cuda(), "src": torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")}
        t.update((k, torch.zeros(size, dtype=torch.uint8, device="cuda")) for k, size in sizes)
        t["dst"] = torch.empty_like(t["src"])
        sets.append(t)
    turn = [0]

    def launch():
        t = sets[turn[0] % SETS]
        turn[0] += 1
        calls.decode_rows_device(ctx, t["rows"], t["off"], t["len"], t["rounds"], t["sigs"], t["sig_len"], t["prev"],
                                 t["prev_len"], t["ok"], sig_stride=96, prev_stride=96)

    def copy():
        t = sets[turn[0] % SETS]
        turn[0] += 1
        t["dst"].copy_(t["src"])

    def timed(f):
        for _ in range(SETS):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps
    runs = [(timed(launch), timed(copy)) for _ in range(3)]
    assert all(int(t["ok"].sum()) == n for t in sets)
    print(f"k_ingest_rows alone: {n} rows, {buf.size} row bytes, {moved} bytes moved per launch, {reps} launches per "
          f"timing over {SETS} buffer sets in turn")
    for tk, tc in runs:
        print(f"  k_ingest_rows {tk * 1e6:9.1f} us  {n / tk / 1e6:8.1f} M rows/s  {moved / tk / 1e9:7.1f} GB/s moved   |   "
              f"device-to-device copy of {moved // 2} bytes {tc * 1e6:9.1f} us  {2 * (moved // 2) / tc / 1e9:7.1f} GB/s moved")


def host_side_alone(bs, n, window):
    """The host's own work per window, nothing on the GPU: the B+tree scan that
    both paths share, and the scan plus the native decode of the host path."""
    from drand_amd import ingest
    for name, f in (("scan only (window_rows)", ingest.window_rows), ("scan + host decode (window_records)", ingest.window_records)):
        for rep in range(2):
            cpu0, t0 = cpu_seconds(), time.perf_counter()
            for lo in range(1, n + 1, window):
                f(bs, lo, min(n + 1, lo + window))
            el, cpu = time.perf_counter() - t0, cpu_seconds() - cpu0
            print(f"{name:36s} rep {rep}: {n / el / 1e6:7.3f} M rows/s  cpu {cpu / (n / 1e6):6.3f} s per million rows")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=2_000_000)
    ap.add_argument("--window", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=12)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    from bolt_writer import write_bolt
    from drand_amd import _lib, ingest
    from drand_amd.boltstore import BoltStore
    from drand_amd.chain import Verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.sync import check_past_beacons
    from drand_amd.synth import corrupt, make_chain
    n = args.rounds
    c = make_chain(args.seed, n, _lib.SCHEME_CHAINED, seg_len=64)
    bad = corrupt(c, args.seed, rate=0.0)  # one round of every corruption kind
    expect = sorted(int(c.rounds[i]) for i in bad)
    t0 = time.perf_counter()
    rows = marshal_chain(c)
    kv = {struct.pack(">Q", 0): b'{"PreviousSig":null,"Round":0,"Signature":"' + c.genesis.hex().encode() + b'"}'}
    kv.update((struct.pack(">Q", int(r)), row) for r, row in zip(c.rounds, rows))
    window_rows = rows[:min(n, args.window)]
    row_bytes = sum(len(r) for r in rows)
    del rows
    d = tempfile.mkdtemp(prefix="drand_ingest_")
    path = os.path.join(d, "drand.db")
    write_bolt(path, kv)
    del kv
    print(f"{n} chained rounds, {len(bad)} corrupted, {row_bytes / n:.1f} row bytes per round; bolt file of "
          f"{os.path.getsize(path)} bytes written in {time.perf_counter() - t0:.0f} s; windows of {args.window}; "
          f"{torch.cuda.get_device_name(0)}; host decode threads {ingest.DECODE_THREADS}, "
          f"cpus {len(os.sched_getaffinity(0))}")
    bs = BoltStore(path)
    v = Verifier(get_scheme_by_id_with_default("pedersen-bls-chained"))
    try:
        for dec in ("host", "device"):  # warm: key decode, buffers, page cache, both paths
            check_past_beacons(bs, v, c.pk, 10 ** 12, window=args.window, decode=dec)
        for mode, name in ((_lib.MODE_PER_ROUND, "per-round"), (_lib.MODE_RLC, "RLC")):
            for dec in ("host", "device"):  # warm the mode's buffers
                check_past_beacons(bs, v, c.pk, 10 ** 12, window=args.window, mode=mode, decode=dec)
            rates = {"host": [], "device": []}
            for rep in range(args.reps):
                for dec in ("host", "device"):
                    cpu0, t0 = cpu_seconds(), time.perf_counter()
                    faulty = check_past_beacons(bs, v, c.pk, 10 ** 12, window=args.window, mode=mode, decode=dec)
                    el, cpu = time.perf_counter() - t0, cpu_seconds() - cpu0
                    assert sorted(faulty or []) == expect, (dec, name, faulty, expect)
                    rates[dec].append(n / el)
                    print(f"{name:9s} decode={dec:6s} rep {rep}: {n / el / 1e6:7.3f} M rounds/s  {el:6.3f} s  "
                          f"cpu {cpu / (n / 1e6):6.3f} s per million rows")
            h, dv = rates["host"], rates["device"]
            print(f"{name:9s} host {min(h) / 1e6:.3f}..{max(h) / 1e6:.3f}  device {min(dv) / 1e6:.3f}..{max(dv) / 1e6:.3f} "
                  f"M rounds/s; host spread {100 * (max(h) - min(h)) / max(h):.1f} %")
        host_side_alone(bs, n, args.window)
        kernel_alone(v.ctx, window_rows, args.kernel_reps)
    finally:
        bs.close()
        os.remove(path)
        os.rmdir(d)


if __name__ == "__main__":
    main()
