"""One small window per compiled scan layout (J, C2, EX): the table behind the variant matrix
(tests/test_gpu_variant_matrix.py, every k_scan<J, C2, EX, MODE> on the GPU) and its ledger
(tests/test_variant_windows_cpu.py, the planner and the CPU replays).

A row is (name, message, policy, lower, count, (J, C2, EX)).  Under its layout policy the planner
gives the row's layout at least 1,500 of the window's nonces; the window holds at most 6,000
nonces, crosses a digit-count boundary, and starts and ends inside a row of the launch grid (the
lane table's launch is a rectangle of whole rows: it ends inside its lane values).  Two rows may
share a window when it runs two layouts (J = 0 and J = 1; the extra-block kernels).  The
ledger checks all of this against the planner and against the kernel manifests, so a layout
compiled without a row here, or a row whose layout is no longer compiled or no longer planned,
fails without a GPU.

Expected values come from the oracle's hashes of a window (one oracle.hash_range per window,
shared and read-only) and numpy; the jobs of the batch modes are batch_jobs.window_jobs' cut of
the window (whole, halves, overlap, single nonces, the digit crossing, nine short ranges).
"""
import random

import numpy as np

import batch_jobs
from collect_batch_jobs import CAPS, answer, own_targets
from first_batch_jobs import KINDS, first_index, target_of

AUTO, UNIFORM, CLASSIC, LANETABLE = 0, 1, 2, 3
MAX_NONCES = 6000
MIN_IN_LAYOUT = 1500
MODES = range(7)  # min, dump, first, collect, min batch, first-hit batch, collect batch


def _msg(name, mlen):
    rng = random.Random(f"variant-window {name} {mlen}")
    return bytes(rng.randrange(256) for _ in range(mlen))


# Lower bounds are odd distances below a power of ten, so that neither end of a window falls on
# the first or last nonce of a row.
_LOW = (_msg("low", 63), AUTO, 10 ** 4 - 2497, 5000)       # 4 digits: J = 0; 5 digits: J = 1
_EX_A = (_msg("extra-a", 42), AUTO, 10 ** 13 - 2497, 5000)  # (13,0,1) -> (14,0,1)
_EX_B = (_msg("extra-c", 50), AUTO, 10 ** 9 - 2497, 5000)   # (14,0,1) -> (15,0,1)
_M58 = _msg("straddle", 58)

TABLE = [("plain-j0",) + _LOW + ((0, 0, 0),),
         ("plain-j1",) + _LOW + ((1, 0, 0),),
         ("plain-j2", b"", AUTO, 10 ** 9 - 2497, 5000, (2, 0, 0))]
# a one-block message of 4J - 9 bytes puts the loop word at J for 9- and 10-digit nonces
TABLE += [(f"plain-j{J}", bytes([0x60 + J]) * (4 * J - 9), AUTO, 10 ** 9 - 2497, 5000, (J, 0, 0))
          for J in range(3, 14)]
TABLE += [("extra-j13",) + _EX_A + ((13, 0, 1),),
          ("extra-j14",) + _EX_A + ((14, 0, 1),),
          ("extra-j15",) + _EX_B + ((15, 0, 1),),
          ("ktab", _msg("ktab", 120), AUTO, 10 ** 11 - 1503, 4000, (0, 1, 0)),
          ("classic", _M58, CLASSIC, 10 ** 9 - 2497, 5000, (1, 1, 0)),
          ("two-word", _M58, UNIFORM, 10 ** 9 - 2497, 5000, (1, 2, 0)),
          ("lane-table", _msg("lane-table", 61), LANETABLE, 10 ** 6 - 1997, 4000, (1, 3, 0))]
NAMES = [row[0] for row in TABLE]
ROWS = {row[0]: row for row in TABLE}
POLICIES = sorted({row[2] for row in TABLE})
LAYOUTS = {row[5] for row in TABLE}

_hashes = {}


def window_hashes(oracle, row):
    """The oracle's hashes of the row's window: one run per (message, lower, count), shared by
    the rows and tests that use it, read-only."""
    _, m, _, lo, cnt, _ = row
    key = (m, lo, cnt)
    if key not in _hashes:
        h = oracle.hash_range(m, lo, cnt)
        h.setflags(write=False)
        _hashes[key] = h
    return _hashes[key]


def first_targets(h):
    """Three targets of a first-hit search over the hashes: the least minus 1 (nothing qualifies),
    the least (one hit, wherever it lies) and the 1/64 quantile (about 78 hits in 5,000)."""
    s = np.sort(h)
    return [int(s[0]) - 1, int(s[0]), int(s[len(s) // 64])]


def row_jobs(row):
    """[(message, lower, upper)] of the row: batch_jobs.window_jobs' cut of its window."""
    name, m, _, lo, cnt, _ = row
    return [(m, a, b) for a, b in batch_jobs.window_jobs(name, lo, cnt)]


def interleaved(rows):
    """[(row, message, lower, upper)]: the jobs of the rows in turn, so that neighbouring jobs
    differ in message and layout."""
    per = [[(r,) + j for j in row_jobs(r)] for r in rows]
    out = []
    for i in range(max(len(p) for p in per)):
        out += [p[i] for p in per if i < len(p)]
    return out


def partner(row):
    """The row whose jobs share a batch call with this row's: the next row of the table with
    another message."""
    i = NAMES.index(row[0])
    return next(r for r in TABLE[i + 1:] + TABLE[:i] if r[1] != row[1])


def truncated(h):
    """The hashes as libgpuhash_tietest.so keeps them: the top 4 bits, in bits 32..35."""
    return (h >> np.uint64(60)) << np.uint64(32)


def job_hashes(oracle, named_job, tie=False):
    row, _, a, b = named_job
    h = window_hashes(oracle, row)[a - row[3]:b - row[3] + 1]
    return truncated(h) if tie else h


def min_jobs(oracle, named, tie=False):
    """([(message, lower, upper)], [(hash, nonce)]): numpy's argmin, the lowest nonce among equal
    hashes."""
    jobs, want = [], []
    for j in named:
        h = job_hashes(oracle, j, tie)
        i = int(np.argmin(h))
        jobs.append(j[1:])
        want.append((int(h[i]), j[2] + i))
    return jobs, want


def first_jobs(oracle, named):
    """([(message, lower, upper, target)], [(hash, nonce) or None]): job k takes the (k mod 5)-th
    of its own five targets (first_batch_jobs.target_of)."""
    jobs, want = [], []
    for k, j in enumerate(named):
        h = job_hashes(oracle, j)
        t = target_of(h, k % KINDS)
        jobs.append(j[1:] + (t,))
        want.append(first_index(h, j[2], t))
    return jobs, want


def collect_jobs(oracle, named, tie_target=None):
    """([(message, lower, upper, target, cap)], [(total, hits)]): job k takes the (k mod 5)-th of
    its own five targets (collect_batch_jobs.own_targets) and the room (0, 5, 5000)[k mod 3].
    With a tie_target: the truncated hashes, that target for every job and room for every hit."""
    jobs, want = [], []
    for k, j in enumerate(named):
        h = job_hashes(oracle, j, tie_target is not None)
        if tie_target is None:
            t, cap = own_targets(h)[k % 5], CAPS[k % 3]
        else:
            t, cap = tie_target, len(h)
        jobs.append(j[1:] + (t, cap))
        want.append(answer(h, j[2], t, cap))
    return jobs, want
