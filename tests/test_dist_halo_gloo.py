"""The halo exchange of a sharded linked segment over two gloo ranks (CPU):
drand_amd.dist.exchange_halo hands rank 1 the last record and length of rank
0's shard -- the previous signature of rank 1's first round -- and hands rank
0 nothing; a rank whose shard is empty gets nothing either (n = 8 at world 2:
the shards are [0, 8) and [8, 8)); at world 1 there is no collective."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

STRIDE = 96


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _record(g):
    """Record g of the test segment: 96 distinct bytes, and a length that varies."""
    return bytes((7 * g + k) & 0xFF for k in range(STRIDE)), (96, 48, 95, 100)[(g // 4) % 4]


def _packed_last(lo, hi):
    """A rank's contribution: its shard's last record and length, zeros when empty."""
    from drand_amd.dist import halo_len_offset
    off = halo_len_offset(STRIDE)
    t = torch.zeros(off + 4, dtype=torch.uint8)
    if hi > lo:
        rec, ln = _record(hi - 1)
        t[:STRIDE] = torch.tensor(list(rec), dtype=torch.uint8)
        t[off:] = torch.tensor(list(ln.to_bytes(4, "little")), dtype=torch.uint8)
    return t


def _worker(rank, world, port, result_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from drand_amd.dist import exchange_halo, shard_range
    out = []
    for n_total in (21, 8, 9):
        lo, hi = shard_range(n_total, world, rank)
        got = exchange_halo(_packed_last(lo, hi), n_total, world, rank)
        out.append(None if got is None else bytes(got.tolist()).hex())
    with open(os.path.join(result_dir, f"rank{rank}.txt"), "w") as f:
        f.write(repr(out))
    dist.destroy_process_group()


def test_halo_exchange_world2(tmp_path):
    from drand_amd.dist import halo_len_offset, shard_range
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [eval(open(tmp_path / f"rank{r}.txt").read()) for r in range(world)]
    # rank 0: its first round takes the caller's seed
    assert res[0] == [None, None, None]
    off = halo_len_offset(STRIDE)
    assert off == STRIDE  # a packed record is sig_stride + 4 bytes
    for n_total, got in zip((21, 8, 9), res[1]):
        lo, hi = shard_range(n_total, world, 1)
        if hi == lo:  # n = 8: the last shard is empty, no halo
            assert n_total == 8 and got is None
            continue
        rec, ln = _record(lo - 1)  # rank 0's last record
        raw = bytes.fromhex(got)
        assert len(raw) == STRIDE + 4
        assert raw[:STRIDE] == rec and int.from_bytes(raw[off:], "little") == ln
    # both a length within the stride and one above it crossed the exchange unchanged
    assert {_record(shard_range(n, world, 1)[0] - 1)[1] for n in (21, 9)} == {100, 48}


def test_halo_exchange_world1_is_a_no_op():
    """No process group exists here: a collective would raise."""
    from drand_amd.dist import exchange_halo
    assert not dist.is_initialized()
    assert exchange_halo(_packed_last(0, 5), 5, 1, 0) is None
