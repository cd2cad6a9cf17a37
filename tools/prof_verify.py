"""Small driver for rocprofv3 PMC passes: build a chain on the GPU, run the
per-round verify pipeline `--iters` times (inputs resident in HBM)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--mode", type=int, default=0)
    a = ap.parse_args()
    import torch
    from drand_amd import _lib, calls
    from drand_amd.chain import get_context
    from drand_amd.synth import make_chain
    torch.cuda.set_device(0)
    c = make_chain(3, a.rounds, _lib.SCHEME_CHAINED, seg_len=max(1, a.rounds // 16384))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(v).to(dev) for v in c.records()]
    bits = torch.zeros((a.rounds + 7) // 8, dtype=torch.uint8, device=dev)
    ctx = get_context(0)
    calls.set_pubkey(ctx, _lib.SCHEME_CHAINED, c.pk)
    s = torch.cuda.current_stream(dev)
    for _ in range(a.iters):
        calls.verify_batch_device(ctx, _lib.SCHEME_CHAINED, *t, a.mode, 7, bits, None, s)
    torch.cuda.synchronize()
    v = np.unpackbits(bits.cpu().numpy(), bitorder="little")[: a.rounds]
    print("valid", int(v.sum()), "of", a.rounds)


if __name__ == "__main__":
    main()
