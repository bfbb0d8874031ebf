"""The class matrix of the packed-kernel tests (CPU replay and GPU alike): jobs of 5 nonces (4 at
one digit) that between them reach every (message length mod 64, digit count) class of
bitcoin-miner_amd/csrc/pack.h, the one-to-two-block transition of the tail and every position
of the length field.

Messages: every length 0..63, then 64, 65, 119, 120, 127, 128, 1300 and one of 2^20 bytes (the
longest the ABI takes).  Per message and digit count d = 1..20 the job [10^(d-1) - 2, 10^(d-1) + 2]
-- it crosses into d digits -- or [0, 3] for d = 1, and the top of uint64, [2^64-5, 2^64-1].
Expected values come from the oracle's hash of every nonce (oracle.hash_range), and numpy.
"""
import random

import numpy as np

U64 = (1 << 64) - 1
LENGTHS = list(range(64)) + [64, 65, 119, 120, 127, 128, 1300, 1 << 20]
PACKED = 64          # GPUHASH_LAYOUT_PACKED_ALWAYS
MAX_SPAN = 1 << 20   # GPUHASH_PACKED_MAX_SPAN


def ranges():
    out = [(0, 3)]
    out += [(10 ** (d - 1) - 2, 10 ** (d - 1) + 2) for d in range(2, 21)]
    return out + [(U64 - 4, U64)]


def messages():
    rng = random.Random("packed class matrix")
    return [bytes(rng.randrange(256) for _ in range(n)) if n < 4096 else rng.randbytes(n) for n in LENGTHS]


def matrix():
    """[(message, lower, upper)]: ranges innermost, so neighbouring jobs differ in digit count."""
    return [(m, a, b) for m in messages() for a, b in ranges()]


_hashes = {}


def hashes(oracle, jobs):
    """The oracle's hashes of every job's nonces, one uint64 array per job; computed once."""
    key = id(jobs)
    if key not in _hashes:
        _hashes[key] = (jobs, [oracle.hash_range(m, a, b - a + 1) for m, a, b in jobs])
    return _hashes[key][1]


def expected_min(hs, jobs):
    out = []
    for h, (_, a, _) in zip(hs, jobs):
        i = int(np.argmin(h))  # the lowest index among equal values
        out.append((int(h[i]), a + i))
    return out


def quartile_targets(hs):
    """Per job the hash at the 1/4 quantile of its own hashes."""
    return [int(np.sort(h)[len(h) // 4]) for h in hs]


def expected_collect(hs, jobs, targets):
    """[(total, [(hash, nonce)] ascending by nonce)] of jobs that list all their hits."""
    out = []
    for h, (_, a, _), t in zip(hs, jobs, targets):
        idx = np.nonzero(h <= np.uint64(t))[0]
        out.append((int(idx.size), [(int(h[i]), a + int(i)) for i in idx]))
    return out
