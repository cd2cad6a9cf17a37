#!/usr/bin/env python3
"""Threshold recovery timed for a G1-signature group next to the existing
G2-signature group, same process and box, at bench.py configs[4]'s shape
(100k rounds, t = 17, n = 32, 10% of rounds with one invalid partial):

    python tools/recover_g1_vs_g2.py [--rounds 100000] [--steps 5] > profiles/r07/recover_g1_vs_g2.txt

Per scheme: synth.make_recovery_batch, one warm-up call of
dgpu_recover_batch_device (batched check, no statuses), then `steps` calls
each timed with a pair of HIP events on the call's stream; the median is
reported as rounds/s, with the dgpu_stage_times split of one further call
and the mismatches against synth.group_signatures (must be 0).  The
G2-signature group runs first and is the yardstick of the box."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(name, code, args):
    import torch
    from drand_amd import calls, synth
    from drand_amd.chain import get_context
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    grp = synth.make_group(args.seed, args.t, args.n, scheme=code)
    msgs, parts, expect_ok = synth.make_recovery_batch(grp, args.rounds, args.seed, args.bad_rate)
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
    print(f"{name}: {n} rounds, t={grp.t}, n={grp.n}, {m} partials/round of {pb} B, "
          f"{int((~expect_ok).sum())} unrecoverable rounds")
    print(f"  calls (ms): {' '.join('%.1f' % x for x in ms)}   median {med:.1f} ms   {n / med * 1e3:,.0f} rounds/s")
    print(f"  mismatches against group_signatures: {mism}")
    print("  stage split of one profiled call (ms): " +
          ", ".join(f"{k} {v:.1f}" for k, v in stages.items()) + f"   total {sum(stages.values()):.1f}")
    return mism


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100000)
    ap.add_argument("--t", type=int, default=17)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--bad-rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("at least 5 timed calls")
    import torch
    from drand_amd import _lib
    torch.cuda.init()
    print(f"threshold recovery, batched check, device buffers; {torch.cuda.get_device_name(0)}")
    bad = run("pedersen-bls-unchained (G2 signatures, the yardstick)", _lib.SCHEME_UNCHAINED, args)
    bad += run("bls-unchained-on-g1 (G1 signatures)", _lib.SCHEME_UNCHAINED_G1, args)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
