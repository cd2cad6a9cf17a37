"""Argument marshalling for the C ABI (include/drand_gpu.h): one function per
entry point that has more than one caller.

Every function takes `ctx` first -- anything with `.lib` and `.handle`: a
_lib.Context, a _lib.MultiContext, a context borrowed from a multi handle --
then the header's arguments by name and in its order.  Counts, strides and
byte lengths come from the arrays' shapes.  A key or seed given as bytes is
copied into an owned uint8 array (a uint8 array is passed as it is); an empty
seed is passed as (NULL, 0).  The return code is checked against ctx.lib, so
the message of a failed call is the one of the library that failed.

Host forms take numpy arrays, allocate their outputs (`fill=` is the value the
reason and randomness arrays hold before the call: a test passes 0xEE to see an
unwritten slot) and check the verdict bitmap against the reasons.  Device forms
take the caller's tensors, outputs included, and a `stream` (a torch stream, or
None for the legacy default stream); they allocate nothing.  A multi form is
the single form under the multi handle's entry point.
"""
import contextlib
import ctypes
import functools
import math
import secrets
import types

import numpy as np

from . import _lib
from ._lib import ptr

G1_SIG_CODES = (_lib.SCHEME_UNCHAINED_G1, _lib.SCHEME_G1_RFC9380)


def sig_width(code):
    """Signature bytes of a scheme code: 48 on G1, 96 on G2."""
    return 48 if code in G1_SIG_CODES else 96


def key_width(code):
    """Public-key (and commitment) bytes: the other group's, 96 or 48."""
    return 144 - sig_width(code)


def rlc_seed_for(mode, rlc_seed):
    """RLC coefficients must be unpredictable to whoever produced the
    beacons: without an explicit seed, RLC mode draws a fresh 64-bit one per
    call (a known seed lets an attacker choose corruptions that cancel)."""
    if mode == _lib.MODE_RLC and rlc_seed is None:
        return secrets.randbits(64)
    return 0 if rlc_seed is None else int(rlc_seed)


def pack_msgs(msgs, min_width=1):
    """Byte records of any length as fixed-stride rows: ((n, stride) uint8,
    (n,) uint32 lengths), the stride at least min_width."""
    n = len(msgs)
    buf = np.zeros((n, max([min_width] + [len(m) for m in msgs])), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    for i, m in enumerate(msgs):
        if m:
            buf[i, : len(m)] = np.frombuffer(bytes(m), dtype=np.uint8)
        lens[i] = len(m)
    return buf, lens


def check_bitmap(bits, reason):
    """The verdict bitmap (bit i of byte i / 8, 1 = valid) must say what the
    reasons say; returns the reasons."""
    valid = np.unpackbits(bits, bitorder="little")[:len(reason)].astype(bool)
    if not np.array_equal(valid, reason == _lib.REASON_OK):
        raise _lib.DrandGPUError(_lib.DGPU_EINVAL, "verdict bitmap and reasons disagree")
    return reason


def _check(ctx, rc):
    return _lib.check(rc, ctx.lib)


def _u8(b):
    return b if hasattr(b, "ctypes") else np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _seed(b):
    s = _u8(b"" if b is None else b)
    return s, (ptr(s) if s.size else None), s.size


def _verdicts(n, fill):
    return np.zeros((n + 7) // 8, dtype=np.uint8), np.full(n, fill, dtype=np.uint8)


def _stream(stream):
    return ctypes.c_void_p(None if stream is None else stream.cuda_stream)


def _dim(given, t, axis):
    return t.shape[axis] if given is None else given


def _addr(t):
    return t if t is None or isinstance(t, int) else ptr(t)


@contextlib.contextmanager
def profiled(ctx):
    """Stage profiling on for the block; yields the function that returns the
    last profiled call's {stage: ms} (_lib.stage_times of ctx)."""
    _check(ctx, ctx.lib.dgpu_set_profiling(ctx.handle, 1))
    try:
        yield functools.partial(_lib.stage_times, ctx)
    finally:
        _check(ctx, ctx.lib.dgpu_set_profiling(ctx.handle, 0))


def synchronize(ctx):
    _check(ctx, ctx.lib.dgpu_synchronize(ctx.handle))


def multi_context(mctx, k):
    """The k-th device's context of a multi handle, as a `ctx` of the
    functions here: the library and the handle, not owned (the multi handle
    keeps owning it)."""
    h = ctypes.c_void_p()
    _check(mctx, mctx.lib.dgpu_multi_context(mctx.handle, k, ctypes.byref(h)))
    return types.SimpleNamespace(lib=mctx.lib, handle=h)


# ------------------------------------------------------------------ keys, groups, data tools
def set_pubkey(ctx, code, pk):
    pk = _u8(pk)
    _check(ctx, ctx.lib.dgpu_set_pubkey(ctx.handle, code, ptr(pk), pk.size))


def derive_pubkey(ctx, code, sk):
    """sk (int or 32 big-endian bytes) -> the compressed key, as bytes."""
    skb = _u8(sk.to_bytes(32, "big") if isinstance(sk, int) else sk)
    pk = np.zeros(key_width(code), dtype=np.uint8)
    _check(ctx, ctx.lib.dgpu_derive_pubkey(ctx.handle, code, ptr(skb), ptr(pk), pk.size))
    return bytes(pk)


def set_group(ctx, code, t, n, commits, entry="dgpu_set_group"):
    """Install a group's t commitments (a list of bytes): dgpu_set_group for
    48-byte G1 commitments, dgpu_set_group_scheme under a G1-signature scheme,
    and dgpu_set_group_wide for a threshold above 32 (up to DGPU_MAX_THRESHOLD).
    The context holds one group at a time: its key (returned) is recorded on
    the context object as `installed_group`, None while no group is known."""
    buf = _u8(b"".join(commits))
    ctx.installed_group = None
    if t > _lib.NARROW_MAX_T:
        rc = getattr(ctx.lib, entry + "_wide")(ctx.handle, code, t, n, ptr(buf), len(commits[0]))
    elif code in G1_SIG_CODES:
        rc = getattr(ctx.lib, entry + "_scheme")(ctx.handle, code, t, n, ptr(buf), len(commits[0]))
    else:
        rc = getattr(ctx.lib, entry)(ctx.handle, t, n, ptr(buf))
    _check(ctx, rc)
    ctx.installed_group = (code, n, tuple(commits))
    return ctx.installed_group


multi_set_group = functools.partial(set_group, entry="dgpu_multi_set_group")


def sign(ctx, code, sk, msgs, msg_len):
    """sk * H(msg) of the (n, stride) message records: (n, signature bytes)."""
    skb = _u8(sk.to_bytes(32, "big") if isinstance(sk, int) else sk)
    out = np.zeros((msgs.shape[0], sig_width(code)), dtype=np.uint8)
    _check(ctx, ctx.lib.dgpu_sign(ctx.handle, code, ptr(skb), msgs.shape[0], ptr(msgs), msgs.shape[1], ptr(msg_len),
                                  ptr(out)))
    return out


def make_partials_scheme(ctx, code, msgs32, sign_idx, label, shares):
    """msgs32 (nr, 32), sign_idx / label (nr, m) uint32, shares (n_shares x 32
    bytes): the (nr, m, 2 + signature bytes) partials."""
    nr, m = sign_idx.shape
    out = np.zeros((nr, m, 2 + sig_width(code)), dtype=np.uint8)
    _check(ctx, ctx.lib.dgpu_make_partials_scheme(ctx.handle, code, nr, ptr(msgs32), m, ptr(sign_idx), ptr(label),
                                                  ptr(shares), shares.size // 32, ptr(out)))
    return out


# ------------------------------------------------------------------ host forms
def verify_batch(ctx, code, rounds, sigs, sig_len, prev, prev_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None, fill=0):
    """Under the key installed by set_pubkey; reasons."""
    n = len(rounds)
    bits, reason = _verdicts(n, fill)
    _check(ctx, ctx.lib.dgpu_verify_batch(ctx.handle, code, n, ptr(rounds), ptr(sigs), sigs.shape[1], ptr(sig_len),
                                          ptr(prev), prev.shape[1], ptr(prev_len), mode, rlc_seed_for(mode, rlc_seed),
                                          ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason)


def verify_beacons(ctx, code, pk, rounds, sigs, sig_len, prev, prev_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None,
                   fill=0, entry="dgpu_verify_beacons"):
    """Fixed-stride host records; the DGPU_REASON_* code per record."""
    n = len(rounds)
    pk = _u8(pk)
    bits, reason = _verdicts(n, fill)
    _check(ctx, getattr(ctx.lib, entry)(ctx.handle, code, ptr(pk), pk.size, n, ptr(rounds), ptr(sigs), sigs.shape[1],
                                        ptr(sig_len), ptr(prev), prev.shape[1], ptr(prev_len), mode,
                                        rlc_seed_for(mode, rlc_seed), ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason)


verify_multi = functools.partial(verify_beacons, entry="dgpu_verify_multi")


def verify_segment(ctx, code, pk, first_round, sigs, sig_len, seed_prev, mode=_lib.MODE_PER_ROUND, rlc_seed=None,
                   randomness=True, fill=0, entry="dgpu_verify_segment"):
    """sigs (n, stride) with sig_len (n,); (reasons, (n, 32) randomness or None)."""
    n = sigs.shape[0]
    pk = _u8(pk)
    seed, seed_ptr, seed_len = _seed(seed_prev)  # (seed: the array, alive until the call has returned)
    bits, reason = _verdicts(n, fill)
    rand = np.full((n, 32), fill, dtype=np.uint8) if randomness else None
    _check(ctx, getattr(ctx.lib, entry)(ctx.handle, code, ptr(pk), pk.size, int(first_round), n, ptr(sigs),
                                        sigs.shape[1], ptr(sig_len), seed_ptr, seed_len, mode,
                                        rlc_seed_for(mode, rlc_seed), ptr(bits), ptr(reason), ptr(rand)))
    return check_bitmap(bits, reason), rand


verify_segment_multi = functools.partial(verify_segment, entry="dgpu_verify_segment_multi")


def verify_recovered(ctx, code, pk, msgs, msg_len, sigs, sig_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None, fill=0):
    n = msgs.shape[0]
    pk = _u8(pk)
    bits, reason = _verdicts(n, fill)
    _check(ctx, ctx.lib.dgpu_verify_recovered(ctx.handle, code, ptr(pk), pk.size, n, ptr(msgs), msgs.shape[1],
                                              ptr(msg_len), ptr(sigs), sigs.shape[1], ptr(sig_len), mode,
                                              rlc_seed_for(mode, rlc_seed), ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason)


def verify_keyed(ctx, code, keys, key_len, key_idx, msgs, msg_len, sigs, sig_len, mode=_lib.MODE_PER_ROUND,
                 rlc_seed=None, fill=0):
    """keys: the table, n_keys x key_len bytes in one uint8 array."""
    n = len(key_idx)
    bits, reason = _verdicts(n, fill)
    _check(ctx, ctx.lib.dgpu_verify_keyed(ctx.handle, code, keys.size // key_len, ptr(keys), key_len, n, ptr(key_idx),
                                          ptr(msgs), msgs.shape[1], ptr(msg_len), ptr(sigs), sigs.shape[1],
                                          ptr(sig_len), mode, rlc_seed_for(mode, rlc_seed), ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason)


def verify_partials(ctx, msgs32, partials, partial_len, mode=_lib.MODE_PER_ROUND, rlc_seed=None, fill=0):
    """partials (nr, m, stride), partial_len (nr, m); reasons of the nr * m slots."""
    nr, m, stride = partials.shape
    bits, reason = _verdicts(nr * m, fill)
    _check(ctx, ctx.lib.dgpu_verify_partials(ctx.handle, nr, ptr(msgs32), m, ptr(partials), stride, ptr(partial_len),
                                             mode, rlc_seed_for(mode, rlc_seed), ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason)


def recover_batch(ctx, msgs32, partials, partial_len, sig_len=96, statuses=True, entry="dgpu_recover_batch"):
    """As verify_partials; sig_len is the installed group's signature width.
    Returns (out_sigs (nr * sig_len,), ok_bits, partial_valid (nr * m,) or None)."""
    nr, m, stride = partials.shape
    out = np.zeros(nr * sig_len, dtype=np.uint8)
    ok = np.zeros((nr + 7) // 8, dtype=np.uint8)
    pv = np.zeros(nr * m, dtype=np.uint8) if statuses else None
    _check(ctx, getattr(ctx.lib, entry)(ctx.handle, nr, ptr(msgs32), m, ptr(partials), stride, ptr(partial_len),
                                        ptr(out), ptr(ok), ptr(pv)))
    return out, ok, pv


recover_multi = functools.partial(recover_batch, entry="dgpu_recover_multi")


def verify_rows(ctx, code, pk, base, row_off, row_len, sig_stride=96, prev_stride=96, mode=_lib.MODE_PER_ROUND,
                rlc_seed=None, fill=0):
    """Stored rows base[row_off[i]:row_off[i] + row_len[i]]; (reasons, row_ok, rounds)."""
    n = len(row_off)
    pk = _u8(pk)
    bits, reason = _verdicts(n, fill)
    ok = np.full(n, fill, dtype=np.uint8)
    rounds = np.full(n, fill, dtype=np.uint64)
    _check(ctx, ctx.lib.dgpu_verify_rows(ctx.handle, code, ptr(pk), pk.size, n, ptr(base), ptr(row_off), ptr(row_len),
                                         sig_stride, prev_stride, mode, rlc_seed_for(mode, rlc_seed), ptr(rounds),
                                         ptr(ok), ptr(bits), ptr(reason)))
    return check_bitmap(bits, reason), ok, rounds


def check_rows(ctx, code, pk, base, row_off, row_len, keys, sig_stride, prev_stride, mode, rlc_seed, first, count,
               reasons=False, fill=0, entry="dgpu_check_rows"):
    """One window of the chain check.  The lists get room for every position
    and every row (untouched pages of an empty array cost nothing; the library
    copies back the entries there are).  Returns (faulty_pos, faulty_val,
    left_rows), and the reasons or None."""
    n = len(row_off)
    pk = _u8(pk)
    pos = np.empty(count, dtype=np.uint64)
    val = np.empty(count, dtype=np.uint64)
    left = np.empty(n, dtype=np.uint64)
    nf, nl = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    reason = np.full(n, fill, dtype=np.uint8) if reasons else None
    rows = [ptr(a) if n else None for a in (base, row_off, row_len, keys)]
    _check(ctx, getattr(ctx.lib, entry)(ctx.handle, code, ptr(pk), pk.size, n, *rows, sig_stride, prev_stride, mode,
                                        rlc_seed_for(mode, rlc_seed), int(first), count,
                                        ptr(pos) if count else None, ptr(val) if count else None, count, ptr(nf),
                                        ptr(left) if n else None, n, ptr(nl), ptr(reason) if n else None))
    return (pos[:int(nf[0])].copy(), val[:int(nf[0])].copy(), left[:int(nl[0])].copy()), reason


check_rows_multi = functools.partial(check_rows, entry="dgpu_check_rows_multi")


# ------------------------------------------------------------------ device forms
# d_* are device tensors.  n and the strides come from the tensors' shapes
# ((n,), (n, stride)); a caller that holds flat tensors names them.
def verify_batch_device(ctx, code, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, mode, rlc_seed, d_bits, d_reason,
                        stream=None):
    _check(ctx, ctx.lib.dgpu_verify_batch_device(ctx.handle, code, d_rounds.shape[0], ptr(d_rounds), ptr(d_sigs),
                                                 d_sigs.shape[1], ptr(d_sig_len), ptr(d_prev), d_prev.shape[1],
                                                 ptr(d_prev_len), mode, rlc_seed_for(mode, rlc_seed), ptr(d_bits),
                                                 ptr(d_reason), _stream(stream)))


def verify_beacons_device(ctx, code, pk, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, mode, rlc_seed, d_bits,
                          d_reason, stream=None, n=None, sig_stride=None, prev_stride=None):
    pk = _u8(pk)
    _check(ctx, ctx.lib.dgpu_verify_beacons_device(ctx.handle, code, ptr(pk), pk.size, _dim(n, d_rounds, 0),
                                                   ptr(d_rounds), ptr(d_sigs), _dim(sig_stride, d_sigs, 1),
                                                   ptr(d_sig_len), ptr(d_prev), _dim(prev_stride, d_prev, 1),
                                                   ptr(d_prev_len), mode, rlc_seed_for(mode, rlc_seed), ptr(d_bits),
                                                   ptr(d_reason), _stream(stream)))


def verify_keyed_device(ctx, code, keys, key_len, d_key_idx, d_msgs, d_msg_len, d_sigs, d_sig_len, mode, rlc_seed,
                        d_bits, d_reason, stream=None):
    _check(ctx, ctx.lib.dgpu_verify_keyed_device(ctx.handle, code, keys.size // key_len, ptr(keys), key_len,
                                                 d_key_idx.shape[0], ptr(d_key_idx), ptr(d_msgs), d_msgs.shape[1],
                                                 ptr(d_msg_len), ptr(d_sigs), d_sigs.shape[1], ptr(d_sig_len), mode,
                                                 rlc_seed_for(mode, rlc_seed), ptr(d_bits), ptr(d_reason),
                                                 _stream(stream)))


def verify_partials_device(ctx, d_msgs32, d_partials, d_partial_len, mode, rlc_seed, d_bits, d_reason, stream=None):
    nr, m, stride = d_partials.shape
    _check(ctx, ctx.lib.dgpu_verify_partials_device(ctx.handle, nr, ptr(d_msgs32), m, ptr(d_partials), stride,
                                                    ptr(d_partial_len), mode, rlc_seed_for(mode, rlc_seed),
                                                    ptr(d_bits), ptr(d_reason), _stream(stream)))


def recover_batch_device(ctx, d_msgs32, d_partials, d_partial_len, d_out_sigs, d_ok, d_status=None, stream=None):
    nr, m, stride = d_partials.shape
    _check(ctx, ctx.lib.dgpu_recover_batch_device(ctx.handle, nr, ptr(d_msgs32), m, ptr(d_partials), stride,
                                                  ptr(d_partial_len), ptr(d_out_sigs), ptr(d_ok), ptr(d_status),
                                                  _stream(stream)))


def decode_rows_device(ctx, d_rows, d_row_off, d_row_len, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, d_ok,
                       stream=None, sig_stride=None, prev_stride=None):
    _check(ctx, ctx.lib.dgpu_decode_rows_device(ctx.handle, d_row_off.shape[0], ptr(d_rows), math.prod(d_rows.shape),
                                                ptr(d_row_off), ptr(d_row_len), ptr(d_rounds), ptr(d_sigs),
                                                _dim(sig_stride, d_sigs, 1), ptr(d_sig_len), ptr(d_prev),
                                                _dim(prev_stride, d_prev, 1), ptr(d_prev_len), ptr(d_ok),
                                                _stream(stream)))


def verify_segment_device(ctx, code, pk, first_round, d_sigs, d_sig_len, seed_prev, mode, rlc_seed, d_bits,
                          d_reason=None, d_randomness=None, stream=None, n=None, sig_stride=None):
    """seed_prev is host bytes, read before the call returns."""
    pk = _u8(pk)
    seed, seed_ptr, seed_len = _seed(seed_prev)  # (seed: the array, alive until the call has returned)
    _check(ctx, ctx.lib.dgpu_verify_segment_device(ctx.handle, code, ptr(pk), pk.size, int(first_round),
                                                   _dim(n, d_sigs, 0), ptr(d_sigs), _dim(sig_stride, d_sigs, 1),
                                                   ptr(d_sig_len), seed_ptr, seed_len, mode,
                                                   rlc_seed_for(mode, rlc_seed), ptr(d_bits), ptr(d_reason),
                                                   ptr(d_randomness), _stream(stream)))


def verify_segment_shard_device(ctx, code, pk, first_round, d_sigs, d_sig_len, d_halo, d_halo_len, mode, rlc_seed,
                                d_bits, d_reason=None, d_randomness=None, stream=None, n=None, sig_stride=None):
    """d_halo / d_halo_len: tensors, or device addresses (a length packed
    behind its record in one tensor)."""
    pk = _u8(pk)
    _check(ctx, ctx.lib.dgpu_verify_segment_shard_device(ctx.handle, code, ptr(pk), pk.size, int(first_round),
                                                         _dim(n, d_sigs, 0), ptr(d_sigs), _dim(sig_stride, d_sigs, 1),
                                                         ptr(d_sig_len), _addr(d_halo), _addr(d_halo_len), mode,
                                                         rlc_seed_for(mode, rlc_seed), ptr(d_bits), ptr(d_reason),
                                                         ptr(d_randomness), _stream(stream)))


def rlc_root_bytes(ctx, code):
    """Bytes of one RLC root of the scheme."""
    rb = ctx.lib.dgpu_rlc_root_bytes(code)
    _check(ctx, min(rb, 0))
    return rb


def rlc_root_device(ctx, code, pk, d_rounds, d_sigs, d_sig_len, d_prev, d_prev_len, rlc_seed, d_root, stream=None,
                    n=None, sig_stride=None, prev_stride=None):
    pk = _u8(pk)
    _check(ctx, ctx.lib.dgpu_rlc_root_device(ctx.handle, code, ptr(pk), pk.size, _dim(n, d_rounds, 0), ptr(d_rounds),
                                             ptr(d_sigs), _dim(sig_stride, d_sigs, 1), ptr(d_sig_len), ptr(d_prev),
                                             _dim(prev_stride, d_prev, 1), ptr(d_prev_len), int(rlc_seed),
                                             ptr(d_root), _stream(stream)))


def rlc_root_segment_device(ctx, code, pk, first_round, d_sigs, d_sig_len, seed_prev, d_halo, d_halo_len, rlc_seed,
                            d_root, stream=None, n=None, sig_stride=None):
    pk = _u8(pk)
    seed, seed_ptr, seed_len = _seed(seed_prev)  # (seed: the array, alive until the call has returned)
    _check(ctx, ctx.lib.dgpu_rlc_root_segment_device(ctx.handle, code, ptr(pk), pk.size, int(first_round),
                                                     _dim(n, d_sigs, 0), ptr(d_sigs), _dim(sig_stride, d_sigs, 1),
                                                     ptr(d_sig_len), seed_ptr, seed_len, _addr(d_halo),
                                                     _addr(d_halo_len), int(rlc_seed), ptr(d_root), _stream(stream)))


def rlc_finish_device(ctx, n_roots, d_roots, d_bits, d_reason=None, stream=None):
    _check(ctx, ctx.lib.dgpu_rlc_finish_device(ctx.handle, n_roots, ptr(d_roots), ptr(d_bits), ptr(d_reason),
                                               _stream(stream)))
