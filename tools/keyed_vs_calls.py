#!/usr/bin/env python3
"""One keyed call against one single-key call per key (dgpu_verify_keyed vs
dgpu_verify_recovered), in one process, alternating, on the same box.

    python tools/keyed_vs_calls.py [--n 1048576] [--keys 1,8,1024,65536] [--reps 2] [--out FILE]

Per signature group (pedersen-bls-unchained: G2 signatures; bls-unchained-g1-
rfc9380: G1 signatures) and per table size K, n records of 32-byte messages,
record i under key i K / n (the records of a key are contiguous, so the
single-key calls take slices):
  (a) calls     the same records as K dgpu_verify_recovered calls, one per
                key -- the way before the keyed entry points, the baseline.
                Above --max-calls keys only that many calls are made (keys
                spread over the table) and the time is scaled to K: marked
                "extrapolated".
  (b) keyed     one dgpu_verify_keyed call, DGPU_MODE_PER_ROUND
  (c) rlc       one dgpu_verify_keyed call, DGPU_MODE_RLC, on the clean
                records and with 0.1% of the signatures' y flipped
and a 1,000-node identity.unsigned_identities call against 1,000 single calls.
Signatures come from dgpu_make_partials_scheme (one call signs every record
with its key's secret); a table above 1,024 keys repeats 1,024 distinct keys
(the library decodes and groups by table entry, whatever the entries hold;
consecutive single-key calls still change key every call, as distinct keys do).
Wall time of the host-form calls (staging included), seconds; every keyed
call's verdicts are checked.  One untimed keyed call per signature group
comes first (the process's first call pays allocations and first launches).
Stage times (ms) of each keyed call's best repetition follow each block.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drand_amd import _lib, calls, identity, synth  # noqa: E402
from drand_amd.chain import get_context, sign, verify_recovered  # noqa: E402
from drand_amd.scheme import get_scheme_by_id_with_default  # noqa: E402

DISTINCT = 1024
GROUPS = (("G2 signatures", "pedersen-bls-unchained", _lib.SCHEME_UNCHAINED),
          ("G1 signatures", "bls-unchained-g1-rfc9380", _lib.SCHEME_G1_RFC9380))


def derive_keys(ctx, code, count):
    sks = [synth.derive_secret(90000 + j) for j in range(count)]
    keys = np.frombuffer(b"".join(calls.derive_pubkey(ctx, code, sk) for sk in sks), dtype=np.uint8)
    return sks, keys.reshape(count, calls.key_width(code)).copy()


def make_records(ctx, code, sks, n, K):
    """msgs (n, 32), sigs (n, 48 | 96), key_idx (n,), sorted by key."""
    rng = np.random.default_rng(n + K)
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    idx = (np.arange(n, dtype=np.uint64) * K // n).astype(np.uint32)
    signer = (idx % DISTINCT).astype(np.uint32)
    shares = np.frombuffer(b"".join(s.to_bytes(32, "big") for s in sks), dtype=np.uint8).copy()
    zero = np.zeros((n, 1), dtype=np.uint32)
    out = calls.make_partials_scheme(ctx, code, msgs, signer.reshape(n, 1), zero, shares)
    return msgs, np.ascontiguousarray(out[:, 0, 2:]), idx


def keyed_call(ctx, code, table, idx, msgs, sigs, mode, seed):
    n = len(idx)
    ml = np.full(n, 32, dtype=np.uint32)
    sl = np.full(n, sigs.shape[1], dtype=np.uint32)
    t0 = time.perf_counter()
    reason = calls.verify_keyed(ctx, code, table, table.shape[1], idx, msgs, ml, sigs, sl, mode, seed)
    return time.perf_counter() - t0, reason


def single_calls(ctx, code, table, idx, msgs, sigs, K, max_calls):
    """One dgpu_verify_recovered call per key over its slice; returns (seconds scaled to K, calls made, bad)."""
    n = len(idx)
    bounds = np.searchsorted(idx, np.arange(K + 1, dtype=np.uint32))
    picks = np.arange(K) if K <= max_calls else np.unique(np.linspace(0, K - 1, max_calls).astype(np.int64))
    ml = np.full(n, 32, dtype=np.uint32)
    sl = np.full(n, sigs.shape[1], dtype=np.uint32)
    bad = 0
    t0 = time.perf_counter()
    for j in picks:
        lo, hi = int(bounds[j]), int(bounds[j + 1])
        if hi == lo:
            continue
        bad += int(np.count_nonzero(calls.verify_recovered(ctx, code, table[j], msgs[lo:hi], ml[lo:hi], sigs[lo:hi],
                                                            sl[lo:hi])))
    dt = time.perf_counter() - t0
    return dt * K / len(picks), len(picks), bad


def fmt_stages(st):
    return "  ".join(f"{k}={v:.2f}" for k, v in st.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", default="1,8,1024,65536")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-calls", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    import torch
    ctx = get_context(0)
    say(f"keyed_vs_calls: n={args.n} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    say("seconds per whole batch, wall time of the host-form calls; (a) = K single-key calls, the baseline")
    for title, name, code in GROUPS:
        sks, distinct = derive_keys(ctx, code, DISTINCT)
        warm = make_records(ctx, code, sks, args.n, 8)  # untimed: allocations, first launches
        for mode in (0, 1):
            keyed_call(ctx, code, np.ascontiguousarray(distinct[:8]), warm[2], warm[0], warm[1], mode, 1)
        del warm
        for K in [int(k) for k in args.keys.split(",")]:
            table = np.ascontiguousarray(distinct[np.arange(K) % DISTINCT])
            msgs, sigs, idx = make_records(ctx, code, sks, args.n, K)
            rng = np.random.default_rng(K)
            victims = np.sort(rng.choice(args.n, size=max(1, args.n // 1000), replace=False))
            dirty = sigs.copy()
            dirty[victims, 0] ^= 0x20
            expect_dirty = np.zeros(args.n, dtype=np.uint8)
            expect_dirty[victims] = _lib.REASON_PAIRING
            say(f"\n== {title} ({name}), K={K}, n/K={args.n / K:.1f}")
            rows = {"calls": [], "keyed": [], "rlc clean": [], "rlc 0.1% bad": []}
            stages = {}
            note = ""
            for rep in range(args.reps):
                dt, made, bad = single_calls(ctx, code, table, idx, msgs, sigs, K, args.max_calls)
                assert bad == 0
                rows["calls"].append(dt)
                if made < K:
                    note = f"  [(a) extrapolated from {made} of {K} calls]"
                with calls.profiled(ctx) as stage_times:
                    for label, mode, s, expect in (("keyed", 0, sigs, None), ("rlc clean", 1, sigs, None),
                                                   ("rlc 0.1% bad", 1, dirty, expect_dirty)):
                        dt, reason = keyed_call(ctx, code, table, idx, msgs, s, mode, 0x5EED0000 + rep)
                        assert np.array_equal(reason, expect) if expect is not None else not reason.any(), label
                        if not rows[label] or dt < min(rows[label]):
                            stages[label] = stage_times()
                        rows[label].append(dt)
            base = min(rows["calls"])
            for label, v in rows.items():
                say(f"  {label:14s} " + " ".join(f"{x:9.4f}" for x in v) + f"   best {min(v):9.4f} s"
                    f"   {args.n / min(v) / 1e6:7.3f} M records/s   x{base / min(v):7.2f} vs (a)" +
                    (note if label == "calls" else ""))
            for label, st in stages.items():
                say(f"  stages[{label}] ms: {fmt_stages(st)}")
    # identities: one keyed call for the group file's nodes against one call per node
    auth = get_scheme_by_id_with_default("")
    sks = [synth.derive_secret(95000 + j) for j in range(args.nodes)]
    keys = [calls.derive_pubkey(ctx, _lib.SCHEME_CHAINED, sk) for sk in sks]
    nodes = [(k, sign(sk, [identity.identity_hash(k)], auth)[0]) for k, sk in zip(keys, sks)]
    nodes[7] = (nodes[7][0], nodes[8][1])
    say(f"\n== identities: Group.UnsignedIdentities over {args.nodes} nodes (one of them unsigned)")
    for rep in range(args.reps):
        t0 = time.perf_counter()
        one = [n for n in nodes if verify_recovered(auth, n[0], [identity.identity_hash(n[0])], [n[1]])[0]]
        t1 = time.perf_counter()
        batch = identity.unsigned_identities(nodes)
        t2 = time.perf_counter()
        assert one == batch == [nodes[7]]
        say(f"  {args.nodes} single calls {t1 - t0:8.4f} s   one keyed call {t2 - t1:8.4f} s   x{(t1 - t0) / (t2 - t1):7.1f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
