"""What the linked-segment GPU tests share (test_gpu_segment*.py and the
segment tools): the explicit records of the defining property, the segment
and shard calls with sentinel-filled outputs, the golden runs and the
randomness check.  The calls return (rc, reasons, randomness): 0 and the
arrays, or the library's error code and None, None."""
import hashlib

import numpy as np

from conftest import load_golden
from drand_amd import _lib, calls

GOLDEN = {"chained": "chain_chained_s1.json", "unchained": "chain_unchained_s1.json",
          "on_g1": "chain_on_g1_s1.json", "g1_rfc9380": "chain_g1_rfc9380_s2.json"}
DEFAULTS = {"DGPU_THR_MIN": "65536", "DGPU_RLC_MIN": "131072", "DGPU_COF_ENGINE_MAX": "16384",
            "DGPU_FE_GS_MAX": "16384"}
FILL = 0xEE  # what reasons and randomness hold before a call: an unwritten slot shows


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    """A numpy array on the GPU (unsigned 32- and 64-bit ones through their signed views)."""
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(dev())


def verdict_tensors(n, rand=True):
    """(bits, reasons, randomness) device outputs, the last two sentinel-filled."""
    import torch
    return (torch.zeros((n + 7) // 8, dtype=torch.uint8, device=dev()),
            torch.full((n,), FILL, dtype=torch.uint8, device=dev()),
            torch.full((n, 32), FILL, dtype=torch.uint8, device=dev()) if rand else None)


def read_verdicts(bits, reason, rand=None):
    """(0, reasons, randomness) on the host, the bitmap checked against the reasons."""
    r = calls.check_bitmap(bits.cpu().numpy(), reason.cpu().numpy())
    return 0, r, None if rand is None else rand.cpu().numpy()


def rc_of(fn):
    """fn()'s (rc, reasons, randomness): a failed call's code in place of the exception."""
    try:
        return fn()
    except _lib.DrandGPUError as e:
        return e.code, None, None


def shifted(first_round, sigs, sig_len, halo, halo_len=None):
    """The explicit records of the defining property: prev[0] is the seed (or
    the halo record with its stated length, which may differ from what it holds)."""
    n, stride = sigs.shape
    halo_len = len(halo) if halo_len is None else halo_len
    rounds = (np.uint64(first_round) + np.arange(n, dtype=np.uint64)).astype(np.uint64)
    prev = np.zeros((n, stride), dtype=np.uint8)
    prev_len = np.zeros(n, dtype=np.uint32)
    held = min(halo_len, stride, len(halo))
    prev[0, :held] = u8(halo)[:held]
    prev_len[0] = halo_len
    prev[1:] = sigs[:-1]
    prev_len[1:] = sig_len[:-1]
    return rounds, prev, prev_len


def explicit_device(ctx, code, pk, first_round, sigs, sig_len, halo, halo_len=None, mode=0, rlc_seed=0):
    """Reasons of dgpu_verify_beacons_device on the shifted records: the reference of the defining property."""
    import torch
    rounds, prev, prev_len = shifted(first_round, sigs, sig_len, halo, halo_len)
    t = [to_dev(a) for a in (rounds, sigs, sig_len, prev, prev_len)]
    bits, reason, _ = verdict_tensors(sigs.shape[0], rand=False)
    torch.cuda.synchronize()
    calls.verify_beacons_device(ctx, code, pk, *t, mode, rlc_seed, bits, reason)
    torch.cuda.synchronize()
    return reason.cpu().numpy()


def segment_host(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0, rand=True):
    return rc_of(lambda: (0,) + calls.verify_segment(ctx, code, pk, first_round, sigs, sig_len, seed, mode, rlc_seed,
                                                     randomness=rand, fill=FILL))


def segment_device(ctx, code, pk, first_round, sigs, sig_len, seed, mode=0, rlc_seed=0):
    import torch
    ts, tl = to_dev(sigs), to_dev(sig_len)
    out = verdict_tensors(sigs.shape[0])
    sd = u8(seed)  # the caller's own buffer (passed as it is), overwritten as soon as the call returns
    torch.cuda.synchronize()

    def run():
        try:
            calls.verify_segment_device(ctx, code, pk, first_round, ts, tl, sd, mode, rlc_seed, *out)
        finally:
            sd[:] = 0xFF  # the seed does not outlive the call in caller memory
        calls.synchronize(ctx)
        torch.cuda.synchronize()
        return read_verdicts(*out)
    return rc_of(run)


def halo_tensor(halo, halo_len, stride):
    """The halo record as the call reads it: min(halo_len, stride) bytes of
    `halo` at the front of a stride-byte record (the rest 0xA5: bytes past the
    length must not matter), and the length, as two device tensors."""
    rec = np.full(stride, 0xA5, dtype=np.uint8)
    held = min(halo_len, stride, len(halo))
    rec[:held] = u8(halo)[:held]
    return to_dev(rec), to_dev(np.array([halo_len], dtype=np.uint32))


def shard_device(ctx, code, pk, first_round, sigs, sig_len, halo, halo_len, mode=0, rlc_seed=0, null_halo=False):
    """The shard call on the NULL stream."""
    import torch
    ts, tl = to_dev(sigs), to_dev(sig_len)
    th, thl = (None, None) if null_halo else halo_tensor(halo, halo_len, sigs.shape[1])
    out = verdict_tensors(sigs.shape[0])
    torch.cuda.synchronize()

    def run():
        calls.verify_segment_shard_device(ctx, code, pk, first_round, ts, tl, th, thl, mode, rlc_seed, *out)
        calls.synchronize(ctx)
        torch.cuda.synchronize()
        return read_verdicts(*out)
    return rc_of(run)


def check_randomness(out, sigs, sig_len, reason):
    """SHA-256 of the signature where the round verifies, zeros elsewhere."""
    for i in range(len(reason)):
        want = hashlib.sha256(bytes(sigs[i, :sig_len[i]])).digest() if reason[i] == 0 else bytes(32)
        assert bytes(out[i]) == want, i


def golden_run(name):
    """(fixture, code, pk, first round, sigs, sig_len, seed) of a golden chain."""
    from drand_amd.scheme import get_scheme_by_id_with_default, scheme_code
    g = load_golden(GOLDEN[name])
    rs = g["rounds"]
    assert [r["round"] for r in rs] == list(range(rs[0]["round"], rs[0]["round"] + len(rs)))
    code = scheme_code(get_scheme_by_id_with_default(g["scheme"]))
    sigs = np.stack([u8(bytes.fromhex(r["sig"])) for r in rs])
    sig_len = np.full(len(rs), len(rs[0]["sig"]) // 2, dtype=np.uint32)
    return g, code, bytes.fromhex(g["pk"]), rs[0]["round"], sigs, sig_len, bytes.fromhex(rs[0]["prev"])


def corrupted_chain(seed, n, code):
    """A chain in 64-round generator segments, whose starts fail in the linked
    view by construction, with every corruption kind the linked form has an
    array for, one sig_len above the stride and one sig_len = 0.  Returns
    (chain, expected-invalid set by construction, index of the over-long record)."""
    from drand_amd import synth
    c = synth.make_chain(seed, n, code, seg_len=64)
    kinds = tuple(k for k in synth.ALL_CORRUPTIONS if k != synth.CORRUPT_PREV)
    bad = synth.corrupt(c, seed, rate=4e-3, kinds=kinds)
    free = [i for i in range(3, n - 3) if not any(j in bad for j in range(i - 2, i + 3))]
    over, zero = free[len(free) // 3], free[2 * len(free) // 3]
    c.sig_len[over] = c.sigs.shape[1] + 1
    c.sig_len[zero] = 0
    corrupted = set(bad) | {over, zero}
    invalid = set(corrupted)
    if code == _lib.SCHEME_CHAINED:
        invalid |= {i + 1 for i in corrupted if i + 1 < n}  # the successor hashes the altered record
        invalid |= set(range(64, n, 64))  # generator-segment starts: signed over a 32-byte seed, not the signature before
    return c, invalid, over
