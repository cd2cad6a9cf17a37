#!/usr/bin/env python3
"""Check-chain over a stored chain: the faulty list replayed on the host
against built on the GPU.

One process, one GPU: the chained chain of tools/ingest_rows_vs_host.py
(--rounds rounds, a handful corrupted) is written as a bolt beacon store, then
CheckPastBeacons runs over it in three legs, alternated, --reps times each, in
per-round mode and in RLC mode:
  (a) decode="device", window=--window             the host replay at the recorded window
  (b) decode="device", window = the whole range    the host replay, one window
  (c) decode="device", replay="device", window=None  one dgpu_check_rows call
Legs (a) and (b) are the code as it was; (b) separates the window size's
effect from the device-built list's.  Reported per run: rounds/s, the
process's CPU seconds per million rows (user + system, every thread), the
bytes the verify call copies back per call (dgpu_verify_rows: n/8 + n + n +
8n; dgpu_check_rows: 16 bytes and 16 per faulty entry, 8 per left row) and
dgpu_staging_stats of the last call.  Every run's faulty list must equal the
construction's.

Prints plain text; profiles/r13/check_rows_vs_windows.txt is one run's output.
"""
import argparse
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Counting:
    """A Verifier that records what each row call copies back to the host."""

    def __init__(self, v):
        self.v, self.ctx, self.d2h, self.calls = v, v.ctx, 0, 0

    def reset(self):
        self.d2h, self.calls = 0, 0

    def verify_reasons(self, *a, **k):
        return self.v.verify_reasons(*a, **k)

    def verify_rows(self, pubkey, buf, off, ln, *a, **k):
        n = len(off)
        self.calls += 1
        self.d2h += (n + 7) // 8 + n + n + 8 * n
        return self.v.verify_rows(pubkey, buf, off, ln, *a, **k)

    def check_rows(self, *a, **k):
        pos, val, left = self.v.check_rows(*a, **k)
        self.calls += 1
        self.d2h += 16 + 16 * len(pos) + 8 * len(left)
        return pos, val, left


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=2_000_000)
    ap.add_argument("--window", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=12)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    from bolt_writer import write_bolt
    from drand_amd import _lib
    from drand_amd.boltstore import BoltStore
    from drand_amd.chain import Verifier
    from drand_amd.scheme import get_scheme_by_id_with_default
    from drand_amd.sync import check_past_beacons
    from drand_amd.synth import corrupt, make_chain
    from ingest_rows_vs_host import cpu_seconds, marshal_chain
    n = args.rounds
    c = make_chain(args.seed, n, _lib.SCHEME_CHAINED, seg_len=64)
    bad = corrupt(c, args.seed, rate=0.0)  # one round of every corruption kind
    expect = sorted(int(c.rounds[i]) for i in bad)
    t0 = time.perf_counter()
    rows = marshal_chain(c)
    kv = {struct.pack(">Q", 0): b'{"PreviousSig":null,"Round":0,"Signature":"' + c.genesis.hex().encode() + b'"}'}
    kv.update((struct.pack(">Q", int(r)), row) for r, row in zip(c.rounds, rows))
    del rows
    d = tempfile.mkdtemp(prefix="drand_check_rows_")
    path = os.path.join(d, "drand.db")
    write_bolt(path, kv)
    del kv
    print(f"{n} chained rounds, {len(bad)} corrupted; bolt file of {os.path.getsize(path)} bytes written in "
          f"{time.perf_counter() - t0:.0f} s; {torch.cuda.get_device_name(0)}; cpus {len(os.sched_getaffinity(0))}; "
          f"one process, one GPU (the several-GPU form is exercised in loopback only and is not measured here)")
    bs = BoltStore(path)
    v = Counting(Verifier(get_scheme_by_id_with_default("pedersen-bls-chained")))
    legs = (("a", f"host replay, window {args.window}", dict(decode="device", window=args.window)),
            ("b", "host replay, one window", dict(decode="device", window=n + 1)),
            ("c", "device replay, one call", dict(decode="device", replay="device", window=None)))
    try:
        for mode, name in ((_lib.MODE_PER_ROUND, "per-round"), (_lib.MODE_RLC, "RLC")):
            for _, _, kw in legs:  # warm: key decode, buffers of this size, page cache
                check_past_beacons(bs, v, c.pk, 10 ** 12, mode=mode, **kw)
            rates = {leg: [] for leg, _, _ in legs}
            for rep in range(args.reps):
                for leg, what, kw in legs:
                    v.reset()
                    cpu0, t0 = cpu_seconds(), time.perf_counter()
                    faulty = check_past_beacons(bs, v, c.pk, 10 ** 12, mode=mode, **kw)
                    el, cpu = time.perf_counter() - t0, cpu_seconds() - cpu0
                    assert sorted(faulty or []) == expect, (leg, name, faulty, expect)
                    rates[leg].append(n / el)
                    dev_ms, host_ms, staged = _lib.staging_stats(v.ctx)
                    print(f"{name:9s} ({leg}) {what:32s} rep {rep}: {n / el / 1e6:7.3f} M rounds/s  {el:6.3f} s  "
                          f"cpu {cpu / (n / 1e6):6.3f} s per million rows  {v.calls} calls, "
                          f"{v.d2h // max(v.calls, 1)} bytes to the host per call; last call staged {staged} bytes in "
                          f"{dev_ms:.1f} ms on the copy stream ({host_ms:.1f} ms host)")
            b, cc = rates["b"], rates["c"]
            spread = (max(b) - min(b)) / max(b)
            print(f"{name:9s} " + "  ".join(f"({leg}) {min(r) / 1e6:.3f}..{max(r) / 1e6:.3f}" for leg, r in rates.items()) +
                  f" M rounds/s; (b) spread {100 * spread:.1f} %; (c) best against (b) best "
                  f"{100 * (max(cc) / max(b) - 1):+.1f} %, (c) worst against (b) worst {100 * (min(cc) / min(b) - 1):+.1f} %")
    finally:
        bs.close()
        os.remove(path)
        os.rmdir(d)


if __name__ == "__main__":
    main()
