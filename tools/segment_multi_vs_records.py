#!/usr/bin/env python3
"""Linked segments across contexts timed next to their counterparts, same
process and box, per-round mode, at the project's A/B size (2M chained rounds
in 64-round generator segments, synth.make_chain):

    DGPU_MULTI_ALLOW_SAME_DEVICE=1 python tools/segment_multi_vs_records.py [--rounds 2000000] \\
        > profiles/r11/segment_multi_vs_records.txt

Pair 1, host arrays, loopback D = 2 (two contexts of one GPU):
dgpu_verify_multi on explicit records (208 staged bytes per round) against
dgpu_verify_segment_multi (signatures alone: 100 bytes per round plus one
halo per later shard, randomness returned).  Pair 2, device-resident chain, one
context: dgpu_verify_segment_device on the whole chain against two
dgpu_verify_segment_shard_device calls on its halves (the second half's halo
is the first half's last record, where it lies in device memory); beside them,
for reference only, the same split with the seed form for both halves, which
tells what splitting one call in two costs whatever the source.

The forms of a pair run alternately, three timed repetitions each after one
untimed call each (allocations, code load).  Per call: wall time as rounds/s,
and for the host pair each context's dgpu_staging_stats bytes (exact).

The counterpart is the yardstick of its pair and the spread between its own
repetitions ((max - min) / mean) the margin: a new path must not be slower
than its counterpart's mean by more than that spread (exit status 1 if one
is).  The expectation is parity, not gain: staging is already hidden
(profiles/r08/segment_vs_records.txt).  In the linked view the
generator-segment starts fail by construction, which costs the per-round path
nothing (it has no early exit).  One GPU: RCCL with real ranks is unmeasured."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REPS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2000000)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    os.environ["DGPU_MULTI_ALLOW_SAME_DEVICE"] = "1"
    import torch
    torch.cuda.init()
    from drand_amd import _lib, calls, synth
    from drand_amd.chain import get_context
    ctx = get_context(0)
    code, n, D = _lib.SCHEME_CHAINED, args.rounds, 2
    c = synth.make_chain(args.seed, n, code, seg_len=64)
    link = c.prev[0, :c.prev_len[0]].copy()
    first = int(c.rounds[0])
    stride = c.sigs.shape[1]
    starts = len(range(64, n, 64))
    shards = [_lib.shard_range(n, D, k) for k in range(D)]
    mctx = _lib.MultiContext([0] * D)
    sub = [calls.multi_context(mctx, k) for k in range(D)]

    def staged():
        return [_lib.staging_stats(s)[2] for s in sub]

    # (the host forms allocate their outputs inside the timed call, as the product's callers do)
    def multi_explicit():
        reason = calls.verify_multi(mctx, code, c.pk, *c.records())
        return int(np.count_nonzero(reason)), [(hi - lo) * (stride + 4 + c.prev.shape[1] + 4 + 8) for lo, hi in shards]

    def multi_linked():
        reason, _ = calls.verify_segment_multi(mctx, code, c.pk, first, c.sigs, c.sig_len, link)
        return int(np.count_nonzero(reason)), [(hi - lo) * (stride + 4) for lo, hi in shards]

    dev = torch.device("cuda", 0)
    d_sigs = torch.from_numpy(c.sigs).to(dev)
    d_len = torch.from_numpy(c.sig_len.view(np.int32)).to(dev)
    d_bits = torch.zeros((n + 7) // 8 + 8, dtype=torch.uint8, device=dev)
    d_reason = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rand = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    half = (n // 2 + 7) & ~7  # whole bitmap bytes in front of the second half

    def invalid_on_device():
        torch.cuda.synchronize()
        return int(torch.count_nonzero(d_reason).item())

    def part(lo, hi):
        """The records [lo, hi) and their outputs, as views of the device arrays."""
        return (d_sigs[lo:hi], d_len[lo:hi]), (d_bits[lo // 8:], d_reason[lo:hi], d_rand[lo:hi])

    def seed_call(lo, hi, seed):
        recs, outs = part(lo, hi)
        calls.verify_segment_device(ctx, code, c.pk, first + lo, *recs, seed, _lib.MODE_PER_ROUND, 0, *outs)

    def whole():
        seed_call(0, n, link)
        return invalid_on_device(), None

    def halves():
        seed_call(0, half, link)
        recs, outs = part(half, n)
        calls.verify_segment_shard_device(ctx, code, c.pk, first + half, *recs, d_sigs[half - 1], d_len[half - 1:half],
                                          _lib.MODE_PER_ROUND, 0, *outs)
        return invalid_on_device(), None

    seed_half = c.sigs[half - 1].copy()  # (the host's copy of the record the shard call reads as its halo)

    def halves_by_seed():
        """The same split with the seed form for both halves: what splitting one call in two costs by itself."""
        seed_call(0, half, link)
        seed_call(half, n, seed_half)
        return invalid_on_device(), None

    print(f"linked segments across contexts vs their counterparts, per-round mode; {n} chained rounds, 64-round "
          f"generator segments; {torch.cuda.get_device_name(0)}")
    bad = slower = 0
    pairs = (("host arrays, loopback D = 2", ("multi explicit", multi_explicit, 0), ("multi linked", multi_linked, starts),
              None, True),
             ("device-resident chain, one context", ("whole segment", whole, starts), ("two shard calls", halves, starts),
              ("two seed calls", halves_by_seed, starts), False))
    for title, base, new, ref, host in pairs:
        print(f"-- {title}")
        forms = (base, new) + ((ref,) if ref else ())
        for _, fn, _ in forms:  # untimed: allocations, code load
            fn()
        rates = {f[0]: [] for f in forms}
        for rep in range(REPS):
            for name, fn, want_invalid in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                invalid, want_bytes = fn()
                dt = time.perf_counter() - t0
                rates[name].append(n / dt)
                ok = invalid == want_invalid
                line = f"  {name:15s} rep {rep}: {dt * 1e3:8.1f} ms  {n / dt:12,.0f} rounds/s   invalid {invalid} " \
                       f"(expected {want_invalid})"
                if host:
                    got = staged()
                    ok = ok and got == want_bytes
                    line += f"   staged bytes per context {got} (expected {want_bytes}; {sum(got) // n} per round)"
                bad += not ok
                print(line + ("" if ok else "   MISMATCH"))
        b, w = rates[base[0]], rates[new[0]]
        b_mean, w_mean = sum(b) / REPS, sum(w) / REPS
        spread = (max(b) - min(b)) / b_mean
        print(f"  {base[0]}: " + ", ".join(f"{x:,.0f}" for x in b) + f" rounds/s, mean {b_mean:,.0f}; spread between "
              f"its repetitions {spread * 100:.2f}%")
        print(f"  {new[0]}: " + ", ".join(f"{x:,.0f}" for x in w) + f" rounds/s, mean {w_mean:,.0f}; "
              f"{(w_mean / b_mean - 1) * 100:+.2f}% against {base[0]}")
        if ref:  # not a condition: tells the cost of the split from the cost of the halo source
            r = rates[ref[0]]
            r_mean = sum(r) / REPS
            print(f"  {ref[0]}: " + ", ".join(f"{x:,.0f}" for x in r) + f" rounds/s, mean {r_mean:,.0f}; "
                  f"{(r_mean / b_mean - 1) * 100:+.2f}% against {base[0]}; {new[0]} {(w_mean / r_mean - 1) * 100:+.2f}% "
                  f"against it")
        is_slower = w_mean < b_mean * (1 - spread)
        slower += is_slower
        print(f"  {new[0]} is " + (f"SLOWER than {base[0]} by more than the spread" if is_slower
                                  else f"not slower than {base[0]} by more than the spread"))
    mctx.close()
    sys.exit(1 if bad or slower else 0)


if __name__ == "__main__":
    main()
