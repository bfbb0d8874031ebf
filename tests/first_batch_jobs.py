"""The jobs of the gpuhash_first_below_batch tests (CPU replay and GPU alike): the job mix of
tests/batch_jobs.py, each job with one of five targets, cycled deterministically over the list:

  0                 nothing qualifies (unless a hash is 0)
  2^64-1            the answer is `lower`
  the least hash    exactly the argmin's lowest nonce
  the median hash   about every second nonce qualifies
  the least - 1     nothing qualifies (unless the least hash is 0)

The mix is listed round-robin over 12 windows, so every window meets every kind of target.
Expected values come from the oracle's hashes of the window: the first index at or below the
target (numpy), what an ascending scan that stops at its first hit returns.
"""
import numpy as np

import batch_jobs
from test_collect_below_cpu import WINDOWS, window_hashes

U64 = (1 << 64) - 1
KINDS = 5


def first_index(h, lo, target):
    idx = np.nonzero(h <= np.uint64(target))[0]
    return None if idx.size == 0 else (int(h[idx[0]]), lo + int(idx[0]))


def job_hashes(oracle, named_job):
    name, m, a, b = named_job
    _, _, _, lo, cnt, _ = {w[0]: w for w in WINDOWS}[name]
    return window_hashes(oracle, name, m, lo, cnt)[a - lo:b - lo + 1]


def target_of(h, kind):
    least = int(h.min())
    return (0, U64, least, int(np.sort(h)[len(h) // 2]), max(least - 1, 0))[kind]


def jobs_and_answers(oracle):
    """([(message, lower, upper, target)], [(hash, nonce) or None]) of the mix."""
    jobs, want = [], []
    for k, named in enumerate(batch_jobs.job_mix()):
        h = job_hashes(oracle, named)
        t = target_of(h, k % KINDS)
        jobs.append((named[1], named[2], named[3], t))
        want.append(first_index(h, named[2], t))
    return jobs, want


def examined(jobs, answers):
    """What gpuhash_last_stats().nonces reports for the batch: per job what an ascending scan
    would have examined, nonce - lower + 1 when found, the span otherwise."""
    return sum((w[1] if w else b) - a + 1 for (_, a, b, _), w in zip(jobs, answers))


def flat(jobs):
    """batch_jobs.flat's arrays and the targets (uint64)."""
    return batch_jobs.flat(jobs) + (np.array([j[3] for j in jobs], dtype=np.uint64),)
