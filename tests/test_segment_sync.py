"""trusted_previous_signature_segments (drand_amd/sync.py): the client walk of
client/verify.go:118-178 over the linked segment form, against the oracle's
restatement (oracle.drand_ref.trusted_previous_signature) on the grid of
targets, points of trust and windows tests/test_sync.py uses for the
per-beacon form.  CPU-only: the verifier is a stand-in whose verify_segment
marks signatures starting with b"BAD" invalid -- and checks what the walk
hands it (one window per call, first round, the seed it links from)."""
import random

import numpy as np
import pytest

from oracle import drand_ref as D


class SegmentStub:
    """Stand-in for chain.Verifier with only verify_segment."""

    def __init__(self, sigs):
        self.sigs = sigs
        self.calls = []

    def verify_segment(self, first_round, sigs, prev_sig, pubkey, mode=0, rlc_seed=None, randomness=True):
        self.calls.append((first_round, len(sigs), prev_sig))
        # the window is the contiguous run it claims to be, linked from the signature before it
        assert list(sigs) == [self.sigs[first_round + k] for k in range(len(sigs))]
        assert not randomness, "the walk consumes no randomness"
        return np.array([3 if s.startswith(b"BAD") else 0 for s in sigs], dtype=np.uint8), None


def _fetch(sigs, log):
    def get_signatures(lo, hi):
        log.append((lo, hi))
        return [sigs[r] for r in range(lo, hi + 1)]
    return get_signatures


@pytest.mark.parametrize("window", [1, 3, 1 << 14])
def test_segment_walk_matches_oracle(window):
    from drand_amd.chain import VerifyError
    from drand_amd.sync import trusted_previous_signature_segments
    rng = random.Random(window)
    errors = 0
    for trial in range(40):
        n = rng.randint(1, 30)
        sigs = {r: (b"BAD" if rng.random() < 0.03 else b"ok") + bytes([r]) for r in range(1, n + 2)}
        pot = rng.choice([None, (rng.randint(1, n), None)])
        if pot:
            pot = (pot[0], sigs[pot[0]])
        target = rng.randint(1, n + 1)
        ref_round = None
        try:
            ref = D.trusted_previous_signature(lambda r, p, s: not s.startswith(b"BAD"), sigs.__getitem__,
                                               b"seed", target, pot)
        except ValueError as e:
            ref, ref_round = "error", int(str(e).rsplit(" ", 1)[1])
        stub, fetched = SegmentStub(sigs), []
        pot_before = pot
        try:
            got = trusted_previous_signature_segments(stub, b"pk", _fetch(sigs, fetched), b"seed", target, pot,
                                                      window=window)
        except VerifyError as e:
            got = "error"
            errors += 1
            assert e.round == ref_round  # the first failure, where the reference returns "verifying beacon"
            assert pot == pot_before     # the caller's point of trust is untouched
        assert got == ref
        # one fetch and one verify per window, each window linked from the one before
        assert [(lo, hi - lo + 1) for lo, hi in fetched] == [(c[0], c[1]) for c in stub.calls]
        assert all(hi - lo + 1 <= window for lo, hi in fetched)
        for k, (first, cnt, seed) in enumerate(stub.calls):
            if k:
                assert first == stub.calls[k - 1][0] + stub.calls[k - 1][1] and seed == sigs[first - 1]


def test_segment_walk_first_failure_round_and_untouched_trust():
    from drand_amd.chain import VerifyError
    from drand_amd.sync import trusted_previous_signature_segments
    sigs = {r: b"ok" + bytes([r]) for r in range(1, 40)}
    sigs[17] = b"BAD17"
    sigs[23] = b"BAD23"
    pot = (5, sigs[5])
    for window in (1, 4, 11, 1 << 14):
        stub = SegmentStub(sigs)
        with pytest.raises(VerifyError) as ei:
            trusted_previous_signature_segments(stub, b"pk", _fetch(sigs, []), b"seed", 30, pot, window=window)
        assert ei.value.round == 17 and ei.value.reason == 3
        assert pot == (5, sigs[5])
        assert stub.calls[0][0] == 6 and stub.calls[0][2] == sigs[5]
    # a target before the failure: the walk succeeds and moves the point of trust
    prev, new_pot = trusted_previous_signature_segments(SegmentStub(sigs), b"pk", _fetch(sigs, []), b"seed", 17, pot,
                                                        window=4)
    assert prev == sigs[16] and new_pot == (16, sigs[16])
    # round 1: the genesis seed, nothing fetched
    log = []
    assert trusted_previous_signature_segments(SegmentStub(sigs), b"pk", _fetch(sigs, log), b"seed", 1, pot) == (b"seed", pot)
    assert log == []
    # a short fetch is an error, not a silent partial walk
    with pytest.raises(ValueError):
        trusted_previous_signature_segments(SegmentStub(sigs), b"pk", lambda lo, hi: [sigs[lo]], b"seed", 30, pot)
