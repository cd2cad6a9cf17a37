#!/usr/bin/env python3
"""Threshold recovery above t = 32 (dgpu_set_group_wide, recover_wide.cuh)
timed next to the narrow path, same process and box, for both signature groups:

    python tools/recover_wide_bench.py [--ts 32,33,65,129,513,1024] [--steps 5] > profiles/<dir>/recover_wide_bench.txt

Per (scheme, t): a group of n = 2 t - 1 nodes (the largest n with
key.MinimumT(n) = t; n = 40 at t = 32), synth.make_recovery_batch with 10% of
rounds unrecoverable, sized to fill the window tables' budget `--fill` times
(RECW_TABLE_BUDGET / (bytes per term * t) rounds per chunk), one warm-up call
of dgpu_recover_batch_device (batched check, no statuses), then `steps` calls
each timed with a pair of HIP events; the median as rounds/s and partials/s,
the dgpu_stage_times split of one further call, and the mismatches against
synth.group_signatures (must be 0).

The yardstick is the reference's stand-in as bench.py uses it at t = 17:
oracle/c_ref.recover_batch on `--ref-rounds` rounds of the same partials on
the box's cores.  The C restatement accepts t <= 64 and G2 signatures only.
Above that, one round goes through oracle.drand_ref.recover (py_yardstick
below says what that figure leaves out); for the G1-signature group the oracle
has no restatement and the tool says so."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

C_REF_MAX_T = 64


def run(name, code, t, args):
    import torch
    from drand_amd import _lib, calls, synth
    from drand_amd.chain import get_context
    TERM_BYTES, BUDGET = _lib.RECW_TERM_BYTES, _lib.RECW_TABLE_BUDGET
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    g1 = code in calls.G1_SIG_CODES
    n_group = 40 if t == 32 else 2 * t - 1
    per_chunk = max(1, BUDGET // (TERM_BYTES[g1] * t))
    rounds = args.rounds or min(int(args.fill * per_chunk) + 1, max(1, args.max_partials // t))
    grp = synth.make_group(args.seed, t, n_group, scheme=code)
    msgs, parts, expect_ok = synth.make_recovery_batch(grp, rounds, args.seed, args.bad_rate)
    expect = synth.group_signatures(grp, msgs)
    n, m, pb = parts.shape
    sb = expect.shape[1]
    calls.set_group(ctx, code, grp.t, grp.n, grp.commits)
    d_msgs = torch.from_numpy(msgs).to(dev)
    d_parts = torch.from_numpy(parts).to(dev)
    d_plen = torch.full((n, m), pb, dtype=torch.int32, device=dev)
    d_out = torch.zeros((n, sb), dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def step():
        calls.recover_batch_device(ctx, d_msgs, d_parts, d_plen, d_out, d_ok, None, stream)

    step()  # warm-up: allocations, code load
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        step()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    with calls.profiled(ctx) as stage_times:
        step()
        torch.cuda.synchronize()
        stages = stage_times()
    ok = d_ok.cpu().numpy().astype(bool)
    out = d_out.cpu().numpy()
    both = ok & expect_ok
    mism = int((ok != expect_ok).sum()) + int((out[both] != expect[both]).any(axis=1).sum()) + int(out[~ok].any())
    med = statistics.median(ms)
    rps = n / med * 1e3
    entry = "dgpu_set_group_wide" if t > _lib.NARROW_MAX_T else "dgpu_set_group[_scheme]"
    print(f"{name} t={t} n={grp.n} ({entry}): {n} rounds of {m} partials ({pb} B), "
          f"{(n + per_chunk - 1) // per_chunk if t > _lib.NARROW_MAX_T else 1} table chunk(s), {int((~expect_ok).sum())} unrecoverable rounds")
    print(f"  calls (ms): {' '.join('%.1f' % x for x in ms)}   median {med:.1f} ms   {rps:,.0f} rounds/s   "
          f"{rps * m:,.0f} partials/s")
    print(f"  mismatches against group_signatures: {mism}")
    print("  stage split of one profiled call (ms): " +
          ", ".join(f"{k} {v:.1f}" for k, v in stages.items()) + f"   total {sum(stages.values()):.1f}")
    if not g1 and t <= C_REF_MAX_T and args.ref_rounds:
        from oracle import c_ref
        k = min(args.ref_rounds, n)
        threads = int(os.environ.get("OMP_NUM_THREADS", "16"))
        t0 = time.perf_counter()
        rsig, rok = c_ref.recover_batch(grp.commits, t, msgs[:k], parts[:k], threads)
        dt = time.perf_counter() - t0
        agree = bool((rok == ok[:k]).all() and (rsig[rok] == out[:k][rok]).all())
        print(f"  yardstick oracle/c_ref.recover_batch: {k} rounds on {threads} threads in {dt:.2f} s = {k / dt:,.1f} rounds/s"
              f"   agrees: {agree}   GPU / yardstick: {rps / (k / dt):,.1f}x")
        mism += 0 if agree else 1
    elif not g1:
        mism += py_yardstick(grp, t, msgs, parts, expect_ok, out, rps, args)
    else:
        print("  yardstick: none -- the oracle restates kyber's tbls.Recover for G2 signatures only (oracle/c "
              "ref_recover, oracle/drand_ref.recover); the reference runs the same Recover with the groups swapped, "
              "so the G2 rows' ratios are the nearest figure")
    del d_msgs, d_parts, d_plen, d_out, d_ok
    return mism


_PY_TERM_S = []  # seconds per term of the Python restatement, as measured (the last is used to extrapolate)


def py_yardstick(grp, t, msgs, parts, expect_ok, out, rps, args):
    """Above the C restatement's t <= 64: oracle.drand_ref.recover on one
    recoverable round of the same partials, VerifyPartial replaced by a stub
    that accepts every partial of that round (all are valid by construction;
    oracle/cpu_baseline.py puts the C pairing there), so the figure leaves the
    reference's t pairings out and favours the yardstick.  One core, scaled to
    the box's cores as if perfectly parallel.  The restatement is linear in t
    (t decompressions, t scalar multiplications), so above --py-ref-max-t the
    per-term cost measured at the largest sampled t is extrapolated and marked
    as such."""
    from oracle import drand_ref as D
    cores = int(os.environ.get("OMP_NUM_THREADS", "16"))
    if t <= args.py_ref_max_t:
        r = int(expect_ok.argmax())
        plist = [bytes(p) for p in parts[r]]
        t0 = time.perf_counter()
        got = D.recover(None, bytes(msgs[r]), plist, t, grp.n, verify=lambda i, sg: True)
        dt = time.perf_counter() - t0
        _PY_TERM_S.append(dt / t)
        agree = got == bytes(out[r])
        print(f"  yardstick: the C restatement accepts t <= {C_REF_MAX_T}; oracle.drand_ref.recover (Python, VerifyPartial "
              f"stubbed) on 1 round: {dt:.1f} s on one core, {cores / dt:.2f} rounds/s if {cores} cores scaled perfectly"
              f"   agrees: {agree}   GPU / yardstick: {rps / (cores / dt):,.0f}x")
        return 0 if agree else 1
    if _PY_TERM_S:
        dt = _PY_TERM_S[-1] * t
        print(f"  yardstick: not sampled above t = {args.py_ref_max_t} (minutes per round in Python); extrapolated from "
              f"{_PY_TERM_S[-1] * 1e3:.0f} ms per term: {dt:.0f} s per round, {cores / dt:.3f} rounds/s on {cores} cores"
              f"   GPU / yardstick (extrapolated): {rps / (cores / dt):,.0f}x")
    else:
        print(f"  yardstick: not sampled above t = {args.py_ref_max_t}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="32,33,65,129,513,1024")
    ap.add_argument("--fill", type=float, default=2.0, help="table budgets per batch")
    ap.add_argument("--max-partials", type=int, default=800000)
    ap.add_argument("--rounds", type=int, default=0, help="rounds per batch (default: from --fill)")
    ap.add_argument("--ref-rounds", type=int, default=64)
    ap.add_argument("--py-ref-max-t", type=int, default=129,
                    help="largest t at which one round runs through the Python restatement (about 0.25 s per term)")
    ap.add_argument("--bad-rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--schemes", default="g2,g1")
    args = ap.parse_args()
    import torch
    from drand_amd import _lib
    torch.cuda.init()
    print(f"threshold recovery, batched check, device buffers; {torch.cuda.get_device_name(0)}")
    schemes = {"g2": ("pedersen-bls-unchained (G2 signatures)", _lib.SCHEME_UNCHAINED),
               "g1": ("bls-unchained-g1-rfc9380 (G1 signatures)", _lib.SCHEME_G1_RFC9380)}
    bad = 0
    for key in args.schemes.split(","):
        for t in [int(x) for x in args.ts.split(",")]:
            bad += run(schemes[key][0], schemes[key][1], t, args)
            sys.stdout.flush()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
