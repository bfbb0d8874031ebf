"""The jobs of the gpuhash_collect_below_batch tests (CPU replay and GPU alike): the job mix of
tests/batch_jobs.py, each job with a target and a room of its own.

Job k takes the (k mod 5)-th of its OWN five targets -- with its n hashes sorted as s: s[0] - 1
(nothing qualifies), s[0] (one hit), s[min(n - 1, max(n // 1000, 1))], s[n // 64] and 2^64-1 (every
nonce; the index of the third is clamped, for the one-nonce jobs) -- and its room cycles through
(0, 5, 5000): a pure count, a few of the hits, all of them.  Expected values come from the
oracle's hashes of the job's window (test_collect_below_cpu.window_hashes) and numpy.
"""
import numpy as np

import batch_jobs
from test_collect_below_cpu import WINDOWS, window_hashes

U64 = (1 << 64) - 1
CAPS = (0, 5, 5000)


def own_targets(h):
    s = np.sort(h)
    n = len(s)
    return [int(s[0]) - 1, int(s[0]), int(s[min(n - 1, max(n // 1000, 1))]), int(s[n // 64]), U64]


def answer(h, lo, target, cap):
    """(total, [(hash, nonce)] of the lowest min(cap, total) hits, ascending by nonce)."""
    idx = np.nonzero(h <= np.uint64(target))[0]
    return int(idx.size), [(int(h[i]), lo + int(i)) for i in idx[:cap]]


def jobs_and_answers(oracle):
    """([(message, lower, upper, target, cap)], [(total, hits)]) of the mix."""
    win = {w[0]: w for w in WINDOWS}
    jobs, want = [], []
    for k, (name, m, a, b) in enumerate(batch_jobs.job_mix()):
        _, _, _, lo, cnt, _ = win[name]
        h = window_hashes(oracle, name, m, lo, cnt)[a - lo:b - lo + 1]
        t, cap = own_targets(h)[k % 5], CAPS[k % 3]
        jobs.append((m, a, b, t, cap))
        want.append(answer(h, a, t, cap))
    return jobs, want


def flat(jobs):
    """The ABI's flat arrays of (message, lower, upper, target, cap) jobs, as numpy arrays: msgs
    (uint8), msg_off, lower, upper, target, out_off (uint64)."""
    msgs, off, lower, upper = batch_jobs.flat(jobs)
    target = np.array([j[3] for j in jobs], dtype=np.uint64)
    out_off = np.zeros(len(jobs) + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum([j[4] for j in jobs], dtype=np.uint64)
    return msgs, off, lower, upper, target, out_off
