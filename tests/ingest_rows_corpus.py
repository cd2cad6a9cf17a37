"""Stored beacon rows for the row-parser tests (tests/test_ingest_rows_host.py,
tests/test_gpu_ingest_rows.py): canonical Beacon.Marshal rows and every way
of leaving the canonical form that dgpu_ingest_decode distinguishes."""
import random

import numpy as np


def marshal(prev, rnd, sig, case=str.lower):
    """Beacon.Marshal's layout; prev / sig: bytes, or None for JSON null;
    rnd: an int or the literal digits."""
    def field(b):
        return "null" if b is None else '"' + case(b.hex()) + '"'
    return ('{"PreviousSig":%s,"Round":%s,"Signature":%s}' % (field(prev), rnd, field(sig))).encode()


def pack(rows, lead=b""):
    """Rows back to back behind `lead`: (buffer, offsets, lengths)."""
    ln = np.array([len(r) for r in rows], dtype=np.uint32)
    off = (len(lead) + np.concatenate([[0], np.cumsum(ln, dtype=np.uint64)[:-1]])).astype(np.uint64)
    return np.frombuffer(lead + b"".join(rows), dtype=np.uint8).copy(), off, ln


def _mixed(h):
    return "".join(c.upper() if i % 3 == 0 else c for i, c in enumerate(h))


def corpus(sig_stride=96, prev_stride=96, seed=1):
    """[(name, row bytes)] at the given strides."""
    rng = random.Random(seed * 1000 + sig_stride + prev_stride)

    def rb(n):
        return bytes(rng.randrange(256) for _ in range(n))
    sig, prev = rb(min(96, sig_stride)), rb(min(96, prev_stride))
    rows = [("chained", marshal(prev, 1234567, sig)),
            ("unchained-null", marshal(None, 42, sig)),
            ("unchained-empty", marshal(b"", 42, sig)),
            ("null-sig", marshal(prev, 42, None)),
            ("empty-sig", marshal(prev, 42, b"")),
            ("both-null", marshal(None, 7, None)),
            ("short-sig-48", marshal(prev, 9, sig[:48])),
            ("genesis-prev-32", marshal(rb(32), 1, sig)),
            ("upper", marshal(prev, 77, sig, str.upper)),
            ("mixed", marshal(prev, 78, sig, _mixed)),
            ("sig-at-stride", marshal(prev, 5, rb(sig_stride))),
            ("sig-over-stride", marshal(prev, 5, rb(sig_stride + 1))),
            ("prev-at-stride", marshal(rb(prev_stride), 5, sig)),
            ("prev-over-stride", marshal(rb(prev_stride + 1), 5, sig)),
            ("empty-row", b""),
            ("garbage", rb(200)),
            ("whitespace", b'{"PreviousSig": null, "Round": 3, "Signature": "' + sig.hex().encode() + b'"}'),
            ("key-order", b'{"Round":3,"PreviousSig":null,"Signature":"' + sig.hex().encode() + b'"}'),
            ("odd-hex", marshal(prev, 3, sig)[:-3] + b'"}'),
            ("trailing-byte", marshal(prev, 3, sig) + b"\n")]
    for name, digits in (("round-0", "0"), ("round-1", "1"), ("round-max", str(2 ** 64 - 1)),
                         ("round-overflow", str(2 ** 64)), ("round-overflow-last-digit", "18446744073709551625"),
                         ("round-leading-zero", "012"), ("round-00", "00"), ("round-21-digits", "1" * 21),
                         ("round-20-digits-over", "9" * 20), ("round-empty", ""), ("round-negative", "-1")):
        rows.append((name, marshal(prev, digits, sig)))
    base = marshal(prev, 918273645, sig)
    rows += [(f"truncated-{k}", base[:k]) for k in range(len(base) + 1)]
    rows += [(f"deleted-{k}", base[:k] + base[k + 1:]) for k in range(len(base))]
    for c in b'",}g0 ':
        rows += [(f"replaced-{k}-{c:02x}", base[:k] + bytes([c]) + base[k + 1:]) for k in range(len(base))]
    return rows
