"""Node identities: the self-signature check of a group file, in one GPU call.

Mirrors (names, argument meaning, behaviour):
  Identity.Hash()                  key/keys.go:52-56   blake2b-256 of the compressed key (key/group.go:27)
  Identity.ValidSignature()        key/keys.go:60-63   AuthScheme.Verify(Key, Hash(), Signature)
  Group.UnsignedIdentities()       key/group.go:474-482  the nodes whose check fails, in order

AuthScheme (key/curve.go:39) is the BLS scheme with signatures on G2 and keys
on G1 under the default scheme's hash DST, so the calls below run under
"pedersen-bls-chained"'s groups.  Every node has its own key:
unsigned_identities is one dgpu_verify_keyed call with the nodes' keys as the
table.  No CPU fallback: the check runs in libdrand_gpu.so.
"""
import hashlib

from . import _lib
from .chain import verify_keyed
from .scheme import get_scheme_by_id_with_default


def _auth_scheme():
    return get_scheme_by_id_with_default("")


def identity_hash(key_bytes):
    """Identity.Hash: blake2b-256 of the 48-byte compressed key."""
    return hashlib.blake2b(bytes(key_bytes), digest_size=32).digest()


def identity_reasons(nodes, mode=_lib.MODE_PER_ROUND, rlc_seed=None, device=0, ctx=None):
    """The DGPU_REASON_* code of every node's self-signature (0 = valid;
    REASON_KEY: the node's key itself is rejected).  nodes: (key, signature)
    pairs of bytes.  A key that is not 48 bytes long can be no G1 point: it is
    REASON_KEY without reaching the device (a table holds keys of one length).
    ctx: a context of the caller's (default: the device's shared one)."""
    nodes = [(bytes(k), bytes(s or b"")) for k, s in nodes]
    reasons = [_lib.REASON_KEY] * len(nodes)
    sized = [i for i, (k, _) in enumerate(nodes) if len(k) == 48]
    if sized:
        got = verify_keyed(_auth_scheme(), [nodes[i][0] for i in sized], list(range(len(sized))),
                           [identity_hash(nodes[i][0]) for i in sized], [nodes[i][1] for i in sized], mode, rlc_seed,
                           device, ctx)
        for i, r in zip(sized, got):
            reasons[i] = int(r)
    return reasons


def valid_signature(key, sig, device=0, ctx=None):
    """Identity.ValidSignature: True iff the signature verifies under the key
    over the key's hash."""
    return identity_reasons([(key, sig)], device=device, ctx=ctx)[0] == _lib.REASON_OK


def unsigned_identities(nodes, mode=_lib.MODE_PER_ROUND, rlc_seed=None, device=0, ctx=None):
    """Group.UnsignedIdentities: the nodes ((key, signature) pairs) whose
    self-signature does not verify, in order; one keyed call for the group."""
    nodes = list(nodes)
    reasons = identity_reasons(nodes, mode, rlc_seed, device, ctx)
    return [n for n, r in zip(nodes, reasons) if r != _lib.REASON_OK]
