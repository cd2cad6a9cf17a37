"""drand_amd.dist.verify_segment_sharded with two rank processes over gloo
sharing one GPU, in the manner of tests/test_gpu_rlc_ranks.py: each rank
holds its shard's signatures in device memory, one all-gather hands rank 1
rank 0's last record as its halo, rank 0 verifies from the segment's seed and
rank 1 through dgpu_verify_segment_shard_device (per-round mode) or
dgpu_rlc_root_segment_device + the roots' all-gather + dgpu_rlc_finish_device
(RLC mode).  The gathered verdicts and reasons equal the single-context
segment call and the construction: in the linked view every 64-round
generator-segment start fails, every round with a corrupted signature, and the
round after it.  The shard boundary (1504) is no segment start, so rank 1's
first round verifies only through the right halo.

Each rank passes the NULL stream or an explicit torch stream, zero-fills its
outputs with torch and reads them back with no device-wide synchronize
(drand_amd/dist.py orders the exchange by stream waits).  Marked gpu."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEG = 3001, 64


def _chain():
    from drand_amd import _lib, synth
    c = synth.make_chain(73, N, _lib.SCHEME_CHAINED, seg_len=SEG)
    kinds = tuple(k for k in synth.ALL_CORRUPTIONS if k != synth.CORRUPT_PREV)
    bad = synth.corrupt(c, 73, rate=2e-3, kinds=kinds)
    invalid = set(range(SEG, N, SEG)) | set(bad) | {i + 1 for i in bad if i + 1 < N}
    return c, invalid


def _rank(rank, world, port, mode, explicit_stream, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from drand_amd import _lib
        from drand_amd.chain import get_context
        from drand_amd.dist import gather_verdict_bits, shard_range, verify_segment_sharded
        torch.cuda.set_device(0)
        c, _ = _chain()
        lo, hi = shard_range(N, world, rank)
        n = hi - lo
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev) if explicit_stream else None
        work = torch.cuda.default_stream(dev) if stream is None else stream
        with torch.cuda.stream(work):  # the shard arrives, and the outputs are zeroed, on the call's stream
            d_sigs = torch.from_numpy(np.ascontiguousarray(c.sigs[lo:hi])).to(dev, non_blocking=True)
            d_sig_len = torch.from_numpy(np.ascontiguousarray(c.sig_len[lo:hi].view(np.int32))).to(dev, non_blocking=True)
            d_bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=dev)
            d_reason = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            d_rand = None if mode == _lib.MODE_RLC else torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev)
        ctx = get_context(0)
        link = bytes(c.prev[0, :c.prev_len[0]])
        verify_segment_sharded(ctx, _lib.SCHEME_CHAINED, np.frombuffer(c.pk, dtype=np.uint8).copy(), int(c.rounds[0]), N,
                               d_sigs, d_sig_len, link, mode, 1000, d_bits, stream, world, rank, d_reason=d_reason,
                               d_randomness=d_rand)
        with torch.cuda.stream(work):  # read back in stream order, no synchronize
            bits_cpu, reason_cpu = d_bits.cpu(), d_reason.cpu()
            rand_cpu = None if d_rand is None else d_rand.cpu()
        bits = gather_verdict_bits(bits_cpu, n, N, world, rank)
        reasons, rands = [None] * world, [None] * world
        dist.all_gather_object(reasons, reason_cpu.numpy()[:n].tolist())
        dist.all_gather_object(rands, None if rand_cpu is None else rand_cpu.numpy()[:n].tobytes())
        if rank == 0:
            q.put((bits.tolist(), sum(reasons, []), None if rands[0] is None else b"".join(rands)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode_name,explicit_stream", [("MODE_PER_ROUND", False), ("MODE_PER_ROUND", True),
                                                       ("MODE_RLC", False), ("MODE_RLC", True)])
def test_segment_sharded_world2_equals_single(mode_name, explicit_stream):
    import torch.multiprocessing as mp
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.dist import shard_range
    from drand_amd.scheme import get_scheme_by_id_with_default
    mode = getattr(_lib, mode_name)
    c, invalid = _chain()
    lo1 = shard_range(N, 2, 1)[0]
    assert lo1 % SEG != 0 and lo1 not in invalid  # rank 1's first round verifies, through its halo alone
    expect = np.ones(N, dtype=bool)
    expect[sorted(invalid)] = False
    v = Verifier(get_scheme_by_id_with_default("pedersen-bls-chained"))
    single, rand = v.verify_segment(int(c.rounds[0]), c.sigs, bytes(c.prev[0, :c.prev_len[0]]), c.pk, mode, 1000,
                                    sig_len=c.sig_len)
    assert np.array_equal(single == 0, expect)  # by construction
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, mode, explicit_stream, q)) for r in range(2)]
    for p in procs:
        p.start()
    bits, reasons, rands = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert bits == expect.tolist()
    assert reasons == single.tolist()
    if mode == _lib.MODE_PER_ROUND:
        assert rands == rand.tobytes()
