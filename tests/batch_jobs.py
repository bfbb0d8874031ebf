"""The job mix of the gpuhash_min_batch tests (CPU replay and GPU alike), made from the windows
of tests/test_collect_below_cpu.py: every layout family, digit-boundary crossings, tail-digit
launches and the top of uint64, cut into about 200 jobs of at most 5,000 nonces.

Per window: the whole window, its two adjacent halves, a range overlapping both, single-nonce
jobs (its first and last nonce -- 2^64-1 for the windows at the top -- and the power of ten
inside it) and seeded short ranges.  The jobs are listed round-robin over the windows, so that
neighbouring jobs differ in message, length and layout and every variant group sees many job
changes.  Expected values come from the oracle's hashes of the window (one run per window,
shared): numpy's argmin, which returns the lowest index among equal values.
"""
import random

import numpy as np

from test_collect_below_cpu import WINDOWS, window_hashes, window_msg

POLICIES = sorted({w[2] for w in WINDOWS})
SHORT_RANGES = 9


def window_jobs(name, lo, cnt):
    """(lower, upper) of the jobs cut from one window, inclusive."""
    hi = lo + cnt - 1
    half = lo + cnt // 2
    jobs = [(lo, hi), (lo, half), (half + 1, hi), (lo + cnt // 4, lo + 3 * cnt // 4), (lo, lo), (hi, hi)]
    p = 1
    while p <= hi:
        if lo < p <= hi:
            jobs += [(p, p), (p - 1, p)]  # the first nonce of a digit count; the crossing itself
        p *= 10
    rng = random.Random(f"min-batch {name}")
    for _ in range(SHORT_RANGES):
        a = lo + rng.randrange(cnt)
        jobs.append((a, min(hi, a + rng.randrange(600))))
    return jobs


def job_mix():
    """[(window name, message, lower, upper)], interleaved over the windows."""
    per = []
    for name, mlen, _policy, lo, cnt, _must in WINDOWS:
        m = window_msg(name, mlen)
        per.append([(name, m, a, b) for a, b in window_jobs(name, lo, cnt)])
    out = []
    for i in range(max(len(p) for p in per)):
        out += [p[i] for p in per if i < len(p)]
    return out


def expected(oracle, jobs):
    """[(hash, nonce)] of the jobs, from the oracle."""
    win = {w[0]: w for w in WINDOWS}
    out = []
    for name, m, a, b in jobs:
        _, _, _, lo, cnt, _ = win[name]
        h = window_hashes(oracle, name, m, lo, cnt)[a - lo:b - lo + 1]
        i = int(np.argmin(h))
        out.append((int(h[i]), a + i))
    return out


def flat(jobs):
    """The ABI's flat arrays of (message, lower, upper) jobs: msgs, msg_off, lower, upper as
    numpy arrays (msgs uint8, the others uint64)."""
    msgs = b"".join(bytes(j[0]) for j in jobs)
    off = np.zeros(len(jobs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(j[0]) for j in jobs], dtype=np.uint64)
    lower = np.array([j[1] for j in jobs], dtype=np.uint64)
    upper = np.array([j[2] for j in jobs], dtype=np.uint64)
    return np.frombuffer(msgs + b"\0", dtype=np.uint8), off, lower, upper
