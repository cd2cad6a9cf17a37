"""The cases of tests/test_gpu_miller6.py, shared with the CPU check of their
corruption maps (tests/test_miller6_host.py).

synth.corrupt marks at least one round per kind, so with the whole catalog a
chain of six rounds or fewer is corrupted everywhere, and an all-fail kernel
would pass.  Each size therefore takes as many kinds as half its rounds (the
pairing failures first: they are the ones that reach the Miller loop), which
leaves valid rounds beside corrupted ones at every n >= 2.  n = 1 cannot have
both in one call: it runs once clean and once corrupted."""
from drand_amd.synth import (CORRUPT_INFINITY, CORRUPT_OTHER_ROUND, CORRUPT_PREV, CORRUPT_TRUNCATED, CORRUPT_X_BIT,
                             CORRUPT_Y_SIGN)

CHAIN_SEED = 19
RATE = 2e-2
# a 5-round block, the 10-item wave and the 64-lane boundary, each with its successor
SIZES = [1, 5, 6, 10, 11, 21, 64, 65]
KINDS = (CORRUPT_Y_SIGN, CORRUPT_OTHER_ROUND, CORRUPT_PREV, CORRUPT_X_BIT, CORRUPT_INFINITY, CORRUPT_TRUNCATED)


def kinds_for(n):
    return KINDS[:max(1, min(len(KINDS), n // 2))]


def corrupt_seed(n):
    return CHAIN_SEED + n


# (n, corrupted): every size corrupted, and the single round also clean
CASES = [(n, True) for n in SIZES] + [(1, False)]
