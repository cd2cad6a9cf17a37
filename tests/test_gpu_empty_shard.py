"""An empty shard in the RLC shard protocol: its root is
the identity pair, the node check sums it with the others, and its finish
step has nothing to resolve or pack.  Both users of the protocol, on the
golden chained chain's first 9 rounds:

- the handle: D = 3 contexts on one GPU (DGPU_MULTI_ALLOW_SAME_DEVICE=1), so
  the shards hold 8, 1 and 0 rounds; dgpu_verify_multi and
  dgpu_verify_segment_multi, both modes, clean and with round index 8 (the
  whole second shard) corrupted, against the single-context call;
- the per-rank entry points: two contexts of one GPU, one rank with the 9
  rounds and one with none; the roots are exchanged by a device concatenation,
  the finish step on the empty rank returns DGPU_OK and the other rank's
  verdicts equal the single call's.

Marked gpu."""

import contextlib

import numpy as np
import pytest

from conftest import load_golden, open_ctx

pytestmark = pytest.mark.gpu

N = 9


def _sch():
    from drand_amd.scheme import get_scheme_by_id_with_default
    return get_scheme_by_id_with_default("pedersen-bls-chained")


@pytest.fixture(scope="module")
def records():
    """The 9 rounds as fixed-stride records, clean and with round index 8's
    signature altered, and the single-context reasons of both."""
    from drand_amd import _lib
    from drand_amd.chain import Beacon, Verifier, pack_beacons
    g = load_golden("chain_chained_s1.json")
    pk = bytes.fromhex(g["pk"])
    beacons = [Beacon(bytes.fromhex(r["prev"]), r["round"], bytes.fromhex(r["sig"])) for r in g["rounds"][:N]]
    clean = pack_beacons(beacons)
    bad = tuple(a.copy() for a in clean)
    bad[1][8, 40] ^= 0x04
    v = Verifier(_sch())
    single = {}
    for name, rec in (("clean", clean), ("bad", bad)):
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            single[name, mode] = v.verify_records(pk, *rec, mode, 5)
    assert single["clean", _lib.MODE_PER_ROUND].tolist() == [0] * N
    assert (single["bad", _lib.MODE_PER_ROUND] != 0).tolist() == [False] * 8 + [True]
    return pk, beacons, {"clean": clean, "bad": bad}, single


@pytest.mark.parametrize("which", ["clean", "bad"])
def test_empty_rlc_shard_over_the_handle(which, records, monkeypatch):
    from drand_amd import _lib
    from drand_amd.chain import Verifier
    from drand_amd.multi import MultiVerifier
    pk, beacons, recs, single = records
    rounds, sigs, sig_len, prev, prev_len = recs[which]
    assert [_lib.shard_range(N, 3, k) for k in range(3)] == [(0, 8), (8, 9), (9, 9)]
    first, link = beacons[0].round, beacons[0].previous_sig
    monkeypatch.setenv("DGPU_MULTI_ALLOW_SAME_DEVICE", "1")
    mv = MultiVerifier(_sch(), [0, 0, 0])
    v = Verifier(_sch())
    try:
        for mode in (_lib.MODE_PER_ROUND, _lib.MODE_RLC):
            got = mv.verify_records(pk, rounds, sigs, sig_len, prev, prev_len, mode, 5)
            assert got.tolist() == single[which, mode].tolist(), mode
            want, want_rand = v.verify_segment(first, sigs, link, pk, mode, 5, sig_len=sig_len)
            assert (want != 0).tolist() == [False] * 8 + [which == "bad"]
            got, rand = mv.verify_segment(first, sigs, link, pk, mode, 5, sig_len=sig_len)
            assert got.tolist() == want.tolist() and np.array_equal(rand, want_rand), mode
    finally:
        mv.close()


@pytest.mark.parametrize("which", ["clean", "bad"])
def test_empty_shard_in_the_rank_protocol(which, records, gpu_ctx):
    import torch
    from drand_amd import _lib, calls
    from drand_amd.dist import rank_seed
    pk, _, recs, single = records
    rounds, sigs, sig_len, prev, prev_len = recs[which]
    pkb = np.frombuffer(pk, dtype=np.uint8).copy()
    code = _lib.SCHEME_CHAINED
    dev = torch.device("cuda", 0)
    with contextlib.closing(open_ctx({})) as other:
        ranks = [(gpu_ctx, N), (other, 0)]  # rank 0 holds every round, rank 1 none
        rb = calls.rlc_root_bytes(gpu_ctx, code)
        assert rb > 0
        held, roots = [], []
        for r, (ctx, n) in enumerate(ranks):
            t = [torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev)
                 for a in (rounds.view(np.int64), sigs, sig_len.view(np.int32), prev, prev_len.view(np.int32))]
            root = torch.full((rb,), 0xA5, dtype=torch.uint8, device=dev)
            # the NULL stream is the legacy default stream, torch's: the concatenation below is ordered behind it
            calls.rlc_root_device(ctx, code, pkb, *t, rank_seed(1000, r, 2), root)
            held.append(t)
            roots.append(root)
        all_roots = torch.cat(roots)
        d_bits = torch.zeros((N + 7) // 8, dtype=torch.uint8, device=dev)
        d_reason = torch.zeros(N, dtype=torch.uint8, device=dev)
        # the empty rank: nothing to write, NULL outputs
        rc = other.lib.dgpu_rlc_finish_device(other.handle, 2, all_roots.data_ptr(), None, None, None)
        assert rc == _lib.DGPU_OK, other.lib.dgpu_last_error()
        calls.rlc_finish_device(gpu_ctx, 2, all_roots, d_bits, d_reason)
        reasons = d_reason.cpu().numpy()
        bits = np.unpackbits(d_bits.cpu().numpy(), bitorder="little")[:N].astype(bool)
        assert reasons.tolist() == single[which, _lib.MODE_PER_ROUND].tolist()
        assert bits.tolist() == (reasons == 0).tolist()
        # the empty rank's root is the identity pair (Z = 0 in both points): not the fill pattern, and
        # summing it changed nothing -- a clean node passed, a bad one failed on rank 0's round alone
        assert not bool((roots[1] == 0xA5).all())
