"""Multi-GPU sharding for bulk verification.

Rounds shard contiguously across ranks: every stored beacon carries its own
PreviousSig (chain/beacon.go:15), so round verdicts are independent and the
data path needs no collective.  The one exchange step is the result: each
rank's verdict bitmap (and its count of failures) is gathered so the caller
(CheckPastBeacons-style, chain/beacon/sync_manager.go:171-232) can rebuild the
global ascending faulty-round list.  Over RCCL ("nccl" backend) on GPUs, gloo
on CPU tensors in tests.
"""
import numpy as np


def shard_range(n_total, world, rank):
    """Contiguous shard [lo, hi) of n_total items for `rank`: the C ABI's rule
    (dgpu_shard_range, used by dgpu_verify_multi) -- shards of
    ceil(n_total / world) items rounded up to a multiple of 8 (whole bitmap
    bytes), the last one takes the remainder (possibly empty)."""
    world = max(1, world)
    per = -(-n_total // world)
    per = (per + 7) & ~7
    lo = min(n_total, rank * per)
    return lo, min(n_total, lo + per)


def gather_verdict_bits(local_bits, n_local, n_total, world, rank, device=None):
    """All-gather per-rank verdict bitmaps (uint8 tensors, ceil(n_local/8) bytes)
    and return the global boolean verdict vector (numpy) on every rank."""
    import torch
    import torch.distributed as dist
    if world == 1:
        return np.unpackbits(local_bits.cpu().numpy(), bitorder="little")[:n_local].astype(bool)
    sizes = [shard_range(n_total, world, r) for r in range(world)]
    max_bytes = max((hi - lo + 7) // 8 for lo, hi in sizes)
    dev = local_bits.device if device is None else device
    if dist.get_backend() == "gloo":  # CPU collectives (tests, one-GPU rehearsals)
        dev = torch.device("cpu")
    buf = torch.zeros(max_bytes, dtype=torch.uint8, device=dev)
    buf[: local_bits.numel()] = local_bits
    out = [torch.zeros(max_bytes, dtype=torch.uint8, device=dev) for _ in range(world)]
    dist.all_gather(out, buf)
    parts = []
    for (lo, hi), t in zip(sizes, out):
        parts.append(np.unpackbits(t.cpu().numpy(), bitorder="little")[: hi - lo].astype(bool))
    return np.concatenate(parts)


def faulty_rounds(verdicts, first_round):
    """Ascending list of invalid rounds (None if none), like CheckPastBeacons."""
    bad = np.nonzero(~verdicts)[0]
    return [int(first_round + i) for i in bad] or None


def rank_seed(seed, rank, world):
    """The RLC seed rank `rank` uses: SplitMix64(seed ^ 0x5EED * (rank + 1)),
    the per-device derivation of dgpu_verify_multi (multi_gpu.h), so every
    rank draws independent coefficients from one caller seed.  Coefficients
    are keyed on the position inside the shard; with one seed shared by two
    ranks, round i of shard A and round i of shard B would get the same
    coefficient and errors +D / -D there would cancel in the summed node
    (ADVICE r04).  world == 1 keeps the seed."""
    if world <= 1:
        return seed & 0xFFFFFFFFFFFFFFFF
    m = 0xFFFFFFFFFFFFFFFF
    z = ((seed ^ (0x5EED * (rank + 1))) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def verify_rlc_sharded(ctx, code, pk, n, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, seed, d_bits, stream,
                       world, rank, d_reason=None, sig_stride=96, prev_stride=96):
    """RLC mode across ranks through the library's per-rank protocol
    (include/drand_gpu.h dgpu_rlc_root_device / dgpu_rlc_finish_device, the
    multi-process form of dgpu_verify_multi's RLC mode): this rank's shard
    root by bucket MSM, the roots all-gathered over torch.distributed (RCCL
    on GPUs), the node (sum of every rank's root) checked with one pairing on
    every rank, this shard's tree descended only when the node fails.  d_* are
    device tensors of this rank's shard.  `seed` may be the same on every
    rank: each rank derives its own (rank_seed).  `stream`: a torch stream or
    None (the legacy default stream, NULL at the C ABI).  The library's work
    is enqueued on it; the exchange is ordered after it by stream waits
    (torch's current stream waits on `stream` before the collective and
    `stream` waits on the collective's result), never by a device-wide
    synchronize.  Returns nothing: the verdict bits land in d_bits (and
    reasons in d_reason) in `stream` order."""
    import torch
    from . import calls
    rb = calls.rlc_root_bytes(ctx, code)
    dev = d_bits.device
    lib_stream = torch.cuda.default_stream(dev) if stream is None else stream
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.stream(lib_stream):  # root allocated in the library's stream order
        root = torch.empty(rb, dtype=torch.uint8, device=dev)
    calls.rlc_root_device(ctx, code, pk, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, rank_seed(seed, rank, world),
                          root, stream, n=n, sig_stride=sig_stride, prev_stride=prev_stride)
    _finish_rlc_sharded(ctx, root, rb, world, d_bits, d_reason, stream, lib_stream, cur)


def _finish_rlc_sharded(ctx, root, rb, world, d_bits, d_reason, stream, lib_stream, cur):
    """Steps 2-3 of the per-rank RLC protocol: the roots' all-gather (ordered
    against the library's stream by waits) and dgpu_rlc_finish_device."""
    import torch
    import torch.distributed as dist
    from . import calls
    dev = root.device
    if world > 1:
        cur.wait_stream(lib_stream)  # the root is written before the collective reads it
        root.record_stream(cur)
        roots = torch.empty(world * rb, dtype=torch.uint8, device=dev)
        if dist.get_backend() == "gloo":  # CPU collectives (tests): .cpu() waits on the current stream
            out = [torch.empty(rb, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(out, root.cpu())
            roots.copy_(torch.cat(out))
        else:
            dist.all_gather_into_tensor(roots, root)
        lib_stream.wait_stream(cur)  # the gathered roots are complete before the finish step reads them
        roots.record_stream(lib_stream)
    else:
        roots = root
    calls.rlc_finish_device(ctx, world, roots, d_bits, d_reason, stream)


def halo_len_offset(sig_stride):
    """Offset of the 32-bit length in a packed halo record: the stride rounded
    up to a multiple of 4 (sig_stride itself for the 96- and 48-byte strides),
    so a packed record is sig_stride + 4 bytes."""
    return (sig_stride + 3) & ~3


def exchange_halo(last, n_total, world, rank):
    """The halo exchange of a linked segment sharded by shard_range: every
    rank contributes `last`, its shard's last record and that record's length
    packed as one uint8 tensor (sig_stride bytes, then the little-endian
    uint32 length at halo_len_offset; zeros from a rank whose shard is empty),
    in one all-gather.  Returns rank - 1's contribution -- this rank's halo,
    the previous signature of its first round -- or None where there is none:
    rank 0 (its first round takes the caller's seed), an empty shard, and
    world 1 (no collective at all).  Works on whatever tensors the backend
    gathers: CPU under gloo, device under RCCL."""
    import torch
    import torch.distributed as dist
    if world <= 1:
        return None
    out = [torch.empty_like(last) for _ in range(world)]
    dist.all_gather(out, last)
    lo, hi = shard_range(n_total, world, rank)
    if rank == 0 or hi == lo:
        return None
    plo, phi = shard_range(n_total, world, rank - 1)
    # only trailing shards are empty, so a non-empty shard's predecessor holds a record
    assert phi > plo and phi == lo, (plo, phi, lo, hi)
    return out[rank - 1]


def verify_segment_sharded(ctx, code, pk, first_round, n_total, d_sigs, d_sig_len, seed_prev, mode, seed, d_bits,
                           stream, world, rank, d_reason=None, d_randomness=None, sig_stride=96):
    """A linked segment (dgpu_verify_segment's input: first round, one seed,
    the signatures) sharded across ranks by shard_range, each rank holding its
    shard's signatures in device memory: d_sigs / d_sig_len are this rank's
    (n, sig_stride) uint8 and (n,) 32-bit tensors, first_round and seed_prev
    the whole segment's.  One all-gather hands every rank its predecessor's
    last record (exchange_halo; a CPU round trip under gloo); rank 0 verifies
    from the seed, rank k > 0 from that halo, read by the kernels in stream
    order (dgpu_verify_segment_shard_device).  RLC mode runs the per-rank
    protocol (dgpu_rlc_root_segment_device, the roots' all-gather,
    dgpu_rlc_finish_device; `seed` as verify_rlc_sharded's) and returns no
    randomness.  `stream` and the ordering rules are verify_rlc_sharded's:
    stream waits, never a device-wide synchronize.  The verdict bits land in
    d_bits (reasons in d_reason, randomness in d_randomness) in `stream`
    order.  Measured with two ranks on one GPU only; RCCL with two or more
    real ranks is unmeasured."""
    import torch
    from . import _lib, calls
    rlc = mode == _lib.MODE_RLC
    if rlc and d_randomness is not None:
        raise ValueError("the per-rank RLC protocol returns no randomness")
    lo, hi = shard_range(n_total, world, rank)
    n = hi - lo
    dev = d_bits.device
    lib_stream = torch.cuda.default_stream(dev) if stream is None else stream
    cur = torch.cuda.current_stream(dev)
    halo = None
    if world > 1:
        import torch.distributed as dist
        off = halo_len_offset(sig_stride)
        cur.wait_stream(lib_stream)  # the shard's records are written before the exchange reads them
        last = torch.zeros(off + 4, dtype=torch.uint8, device=dev)
        if n:
            last[:sig_stride] = d_sigs.reshape(-1)[(n - 1) * sig_stride:n * sig_stride]
            last[off:] = d_sig_len[n - 1:n].view(torch.uint8)
        gloo = dist.get_backend() == "gloo"  # CPU collectives (tests): .cpu() waits on the current stream
        got = exchange_halo(last.cpu() if gloo else last, n_total, world, rank)
        if got is not None:
            halo = got.to(dev)
            lib_stream.wait_stream(cur)  # the halo is on the device before the library's kernels read it
            halo.record_stream(lib_stream)
    halo_args = (None, None) if halo is None else (halo.data_ptr(), halo.data_ptr() + halo_len_offset(sig_stride))
    first = int(first_round) + lo
    shape = dict(n=n, sig_stride=sig_stride)
    if not rlc:
        if rank == 0 or n == 0:
            calls.verify_segment_device(ctx, code, pk, first, d_sigs, d_sig_len, seed_prev, mode, 0, d_bits, d_reason,
                                        d_randomness, stream, **shape)
        else:
            calls.verify_segment_shard_device(ctx, code, pk, first, d_sigs, d_sig_len, *halo_args, mode, 0, d_bits,
                                              d_reason, d_randomness, stream, **shape)
        return
    rb = calls.rlc_root_bytes(ctx, code)
    with torch.cuda.stream(lib_stream):  # root allocated in the library's stream order
        root = torch.empty(rb, dtype=torch.uint8, device=dev)
    calls.rlc_root_segment_device(ctx, code, pk, first, d_sigs, d_sig_len, seed_prev,
                                  *(halo_args if rank and n else (None, None)), rank_seed(seed, rank, world), root,
                                  stream, **shape)
    # (the halo tensor stays referenced until the finish step has been enqueued)
    _finish_rlc_sharded(ctx, root, rb, world, d_bits, d_reason, stream, lib_stream, cur)
