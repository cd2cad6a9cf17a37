#!/usr/bin/env python3
"""The linked-segment call timed next to the explicit-record call, same
process and box, host records, per-round mode, at the project's A/B size
(2M chained rounds in 64-round generator segments, synth.make_chain):

    python tools/segment_vs_records.py [--rounds 2000000] > profiles/r08/segment_vs_records.txt

dgpu_verify_beacons (rounds, signatures, previous signatures: 208 staged
bytes per round) and dgpu_verify_segment (signatures alone: 100 bytes per
round, randomness returned) run alternately, two timed repetitions each
after one untimed call each (allocations, code load).  Per call: wall time
of the synchronous call as rounds/s, and dgpu_staging_stats (device ms, host
ms, bytes -- the bytes are exact: n x 208 and n x 100).

The explicit call is the yardstick of the run and the spread between its own
two repetitions the margin: the linked form must not be slower than the
explicit form by more than that spread (exit status 1 if it is).  A faster
linked form is a result, not a requirement.  (In the linked call the
generator-segment starts fail by construction -- they were signed over a
32-byte seed, not over the signature before them -- which costs the
per-round path nothing: it has no early exit.)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2000000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-randomness", action="store_true", help="the linked call without its randomness output")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from drand_amd import _lib, calls, synth
    from drand_amd.chain import get_context
    ctx = get_context(0)
    code, n = _lib.SCHEME_CHAINED, args.rounds
    c = synth.make_chain(args.seed, n, code, seg_len=64)
    link = c.prev[0, :c.prev_len[0]].copy()
    stride = c.sigs.shape[1]

    # (both forms allocate their outputs inside the timed call, as the product's callers do)
    def explicit():
        reason = calls.verify_beacons(ctx, code, c.pk, *c.records())
        return int(np.count_nonzero(reason)), n * (stride + 4 + c.prev.shape[1] + 4 + 8)

    def linked():
        reason, _ = calls.verify_segment(ctx, code, c.pk, int(c.rounds[0]), c.sigs, c.sig_len, link,
                                         randomness=not args.no_randomness)
        return int(np.count_nonzero(reason)), n * (stride + 4)

    forms = (("explicit", explicit, 0), ("linked", linked, len(range(64, n, 64))))
    print(f"explicit records vs linked segment, host records, per-round mode; {n} chained rounds, 64-round generator "
          f"segments; {torch.cuda.get_device_name(0)}")
    for _, fn, _ in forms:  # untimed: allocations, code load
        fn()
    rates = {"explicit": [], "linked": []}
    bad = 0
    for rep in range(2):
        for name, fn, want_invalid in forms:
            t0 = time.perf_counter()
            invalid, want_bytes = fn()
            dt = time.perf_counter() - t0
            dev_ms, host_ms, nbytes = _lib.staging_stats(ctx)
            rates[name].append(n / dt)
            ok = invalid == want_invalid and nbytes == want_bytes
            bad += not ok
            print(f"  {name:8s} rep {rep}: {dt * 1e3:8.1f} ms  {n / dt:12,.0f} rounds/s   staging: device {dev_ms:7.1f} ms, "
                  f"host {host_ms:7.1f} ms, {nbytes} bytes ({nbytes // n} per round, expected {want_bytes})   "
                  f"invalid {invalid} (expected {want_invalid}){'' if ok else '   MISMATCH'}")
    e, l = rates["explicit"], rates["linked"]
    e_mean, l_mean = sum(e) / 2, sum(l) / 2
    spread = abs(e[0] - e[1]) / e_mean
    print(f"explicit: {e[0]:,.0f} and {e[1]:,.0f} rounds/s, mean {e_mean:,.0f}; spread between its repetitions "
          f"{spread * 100:.2f}%")
    print(f"linked:   {l[0]:,.0f} and {l[1]:,.0f} rounds/s, mean {l_mean:,.0f}; {(l_mean / e_mean - 1) * 100:+.2f}% "
          f"against explicit")
    slower = l_mean < e_mean * (1 - spread)
    print("linked is " + ("SLOWER than explicit by more than the spread" if slower
                          else "not slower than explicit by more than the spread"))
    sys.exit(1 if bad or slower else 0)


if __name__ == "__main__":
    main()
