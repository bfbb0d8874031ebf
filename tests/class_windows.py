"""Windows that between them reach every (message length mod 64, digit count) class of the scan
kernels: the table behind the class matrix (tests/test_gpu_class_matrix.py, on the GPU) and its
ledger (tests/test_class_windows_cpu.py, the planner and the CPU replay).

A compiled k_scan<J, C2, EX, MODE> serves many arrangements: loop_shift, the lane masks, qmask, R,
R1 and RQ, the place of the 0x80 byte and of the length field in U, the split of the digits
between block B-1 and block B, the extra padding block and the tail-digit stride all follow the
message length mod 64, the digit count and the layout policy (csrc/plan.h, LaunchDesc).  The
variant matrix (tests/variant_windows.py) meets one arrangement per compiled layout; this table
meets all 1,280 classes, 64 residues x 20 digit counts.

Messages: one per length 0..127, seeded random bytes.  Each residue appears twice: below 64
bytes the chaining value that enters the digit blocks is the IV, from 64 bytes on a real midstate.

Windows per message, all inclusive, 45 of them, 67,800 nonces:
  A        [0, 10999]: the digit counts 1 to 4 in full and the bottom of 5
  B5..B19  [10^k - 1249, 10^k + 1250]: the digit-count crossings
  C        [2^64 - 2500, 2^64 - 1]
  D5..D20  [b - 300, b + 299], b a seeded multiple of 10^4 with the window inside the d-digit
           group: the loop digits roll over and the lane value carries into arbitrary digits
  E9..E20  the same with b a multiple of 10^8: the carry from ascii4(p % 10^4) into
           ascii4(p / 10^4)
A D or E window is also cut into 16 pieces (600 is no multiple of 16: they hold 37 or 38 nonces).

Policy runs: AUTO | TAIL_NEVER runs every window; AUTO | TAIL_ALWAYS, UNIFORM | TAIL_NEVER and
LANETABLE | TAIL_NEVER run the windows whose plan differs from the AUTO | TAIL_NEVER plan.  A
(message, window, policy run) that runs is a case.  CLASSIC | TAIL_NEVER plans every window as
AUTO | TAIL_NEVER does (the windows are narrower than two loop values of a J = 1 straddle), and the
tail flag and the layout policy act on different digit groups, so neither adds a case.

Expected values come from the oracle's hashes of a window (one oracle.hash_range per message and
window, shared and read-only) and numpy.  Nothing here needs a GPU or the oracle at import; the
planner (libgpuhash_hostcheck.so) is loaded by load_planner().

No class has needed a regression window yet: the matrix found no mismatch when it was written.
A class that does is recorded here as one line, (message length, window, policy run).
"""
import collections
import ctypes
import os
import random
import subprocess

import numpy as np

from collect_batch_jobs import CAPS, answer, own_targets
from first_batch_jobs import KINDS, first_index, target_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
U64 = (1 << 64) - 1
AUTO, UNIFORM, CLASSIC, LANETABLE, TAIL_ALWAYS, TAIL_NEVER = 0, 1, 2, 3, 16, 32
POLICY_RUNS = (("auto", AUTO | TAIL_NEVER), ("tail", AUTO | TAIL_ALWAYS),
               ("uniform", UNIFORM | TAIL_NEVER), ("lanetable", LANETABLE | TAIL_NEVER))
RUN_NAMES = [name for name, _ in POLICY_RUNS]
POLICY = dict(POLICY_RUNS)
LENGTHS = range(128)
BLOCKS = [range(16 * i, 16 * i + 16) for i in range(8)]  # the GPU cases: 16 message lengths each
# The parts of the GPU matrix, (message lengths, policy runs, (k, n)): per block the three runs
# whose calls cost microseconds, and the UNIFORM run one message length at a time, in shares
# ((k, n) takes every n-th of the length's UNIFORM cases from the k-th on).  Its two-word loop
# (C2 = 2) gives a lane up to 10^8 loop values, so a window of 600 nonces is one row of up to 10^8
# row-iterations, nearly all of them masked: up to 0.17 s per call on an MI355X.  A length runs in
# two halves, the cases at even and at odd places.  (Four shares by place were measured in the
# min-batch mode and are worse: places 0, 4, 8, ... hold all three R = 10^8 windows of a length.)
# UNIFORM plans differently from AUTO only where a J = 1 layout straddles two blocks: lengths
# 48..62 mod 64.
UNIFORM_LENGTHS = [n for n in LENGTHS if 48 <= n % 64 <= 62]
MODES = ("min", "dump", "first", "collect", "min-batch", "first-batch", "collect-batch")
BLOCK_PARTS = [(f"block{i}", (b, ("auto", "tail", "lanetable"), (0, 1))) for i, b in enumerate(BLOCKS)]


def _shares(letters):
    n = len(letters)
    return [(f"uniform{m}{letters[k]}", ((m,), ("uniform",), (k, n))) for m in UNIFORM_LENGTHS for k in range(n)]


def parts_of(mode):
    """[(name, part)] of a mode of the GPU matrix: the same 68 parts in every mode."""
    return BLOCK_PARTS + _shares("ab")


GPU_CASES = [(name, part, mode) for mode in range(len(MODES)) for name, part in parts_of(mode)]
HALF = 300      # nonces on each side of a D or E window's pivot
PIECES = 16


class Info(ctypes.Structure):
    """gpuhash_plan_info of libgpuhash_hostcheck.so (csrc/hostcheck.cpp)."""
    _fields_ = ([(n, ctypes.c_int) for n in "J C2 EX d q s".split()]
                + [(n, ctypes.c_uint64) for n in "lo hi base".split()]
                + [(n, ctypes.c_uint32) for n in "nblocks R rchunk nrchunks p_first p_last r_first r_last".split()]
                + [(n, ctypes.c_uint32) for n in "stride tail".split()])


Window = collections.namedtuple("Window", "name kind lo hi pivot")
Launch = collections.namedtuple("Launch", [f for f, _ in Info._fields_])


def group_of(d):
    """The first and last nonce of d digits."""
    return (0 if d == 1 else 10 ** (d - 1)), min(10 ** d - 1, U64)


def digits(n):
    return len(str(n))


def class_of(mlen, n):
    return mlen % 64, digits(n)


def message(mlen):
    rng = random.Random(f"class-window message {mlen}")
    return bytes(rng.randrange(256) for _ in range(mlen))


MESSAGES = [message(n) for n in LENGTHS]


def _pivot(mlen, d, step):
    """A seeded multiple of `step` strictly inside the d-digit group, HALF nonces of the group on
    each side of it."""
    lo, hi = group_of(d)
    rng = random.Random(f"class-window pivot {mlen} {d} {step}")
    return step * rng.randint(lo // step + 1, (hi - HALF + 1) // step)


def _windows(mlen):
    out = [Window("A", "A", 0, 10999, None)]
    out += [Window(f"B{k}", "B", 10 ** k - 1249, 10 ** k + 1250, 10 ** k) for k in range(5, 20)]
    out.append(Window("C", "C", U64 - 2499, U64, None))
    for kind, first, step in (("D", 5, 10 ** 4), ("E", 9, 10 ** 8)):
        for d in range(first, 21):
            b = _pivot(mlen, d, step)
            out.append(Window(f"{kind}{d}", kind, b - HALF, b + HALF - 1, b))
    return out


WINDOWS = [_windows(n) for n in LENGTHS]   # WINDOWS[mlen]: the 45 windows of that message
WINDOW = [{w.name: w for w in ws} for ws in WINDOWS]
NONCES_PER_MESSAGE = sum(w.hi - w.lo + 1 for w in WINDOWS[0])


def pieces(w):
    """The 16 pieces of a D or E window, [(lower, upper)]: cut at i * 600 // 16."""
    n = w.hi - w.lo + 1
    cuts = [w.lo + i * n // PIECES for i in range(PIECES + 1)]
    return [(a, b - 1) for a, b in zip(cuts, cuts[1:])]


def halves(w):
    mid = w.lo + (w.hi - w.lo + 1) // 2
    return [(w.lo, mid - 1), (mid, w.hi)]


# ---- the planner ----

def load_planner():
    """libgpuhash_hostcheck.so (built when missing or older than its source), with the argument
    types of the entry points the class matrix uses."""
    path = os.path.join(PKG, "lib", "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    u64, u32, cp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p
    lib.gpuhash_plan_count.argtypes = [cp, u64, u64, u64, u32]
    lib.gpuhash_plan_all.argtypes = [cp, u64, u64, u64, u32, ctypes.POINTER(Info), ctypes.c_int]
    lib.hostcheck_desc_hash.argtypes = [cp, u64, u64, u64, u32, ctypes.c_int, u64, ctypes.POINTER(u64)]
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    return lib


_room = (Info * 512)()
_fields = Launch._fields


def plan(hc, m, a, b, policy):
    """The launches of [a, b] under the policy, as Launch tuples.  Leaves the planner's policy set."""
    hc.hostcheck_set_layout_policy(policy)
    n = hc.gpuhash_plan_all(m, len(m), a, b, 0, _room, 512)
    assert 0 < n <= 512, (len(m), a, b, policy, n)
    return [Launch(*[getattr(_room[i], f) for f in _fields]) for i in range(n)]


def nonces(l):
    return (l.hi - l.lo) // l.stride + 1


def layout(l):
    return l.J, l.C2, l.EX


def arrangement(l):
    return l.J, l.C2, l.EX, l.q, l.s, l.stride


def variant_groups(launches):
    """{(J, C2, EX, digits)} as a device run reports its launches (csrc/stage.h): one per kernel
    variant, with the digit count of the variant's largest launch, the first of equals."""
    best = {}
    for l in launches:
        if layout(l) not in best or nonces(l) > best[layout(l)][0]:
            best[layout(l)] = (nonces(l), l.d)
    return {k + (d,) for k, (_, d) in best.items()}


_plans, _cases = {}, {}


def window_plan(hc, mlen, w, run):
    key = (mlen, w.name, run)
    if key not in _plans:
        _plans[key] = plan(hc, MESSAGES[mlen], w.lo, w.hi, POLICY[run])
    return _plans[key]


def run_cases(hc, mlen):
    """[(window, policy run)] of the message: every window under "auto", and under each other run
    the windows whose plan differs from the "auto" plan."""
    if mlen not in _cases:
        out = [(w, "auto") for w in WINDOWS[mlen]]
        for run in RUN_NAMES[1:]:
            out += [(w, run) for w in WINDOWS[mlen] if window_plan(hc, mlen, w, run) != window_plan(hc, mlen, w, "auto")]
        _cases[mlen] = out
    return _cases[mlen]


def part_cases(hc, mlen, run, share=(0, 1)):
    """The windows of a message's cases under one policy run; share (k, n): every n-th from the k-th."""
    return [w for w, r in run_cases(hc, mlen) if r == run][share[0]::share[1]]


def case_jobs(hc, mlen, run, share=(0, 1)):
    """[(window, lower, upper)] of a message's cases under one policy run, for the batch modes:
    each window, and the 16 pieces of each D and E window."""
    out = []
    for w in part_cases(hc, mlen, run, share):
        out.append((w, w.lo, w.hi))
        if w.kind in "DE":
            out += [(w, a, b) for a, b in pieces(w)]
    return out


def block_jobs(hc, block, run, share=(0, 1)):
    """[(message length, window, lower, upper)]: the jobs of a block's messages under one policy
    run, one message after the other in turn, so that neighbouring jobs differ in message (where
    the block holds more than one: a UNIFORM part is one message's)."""
    per = [[(mlen,) + j for j in case_jobs(hc, mlen, run, share)] for mlen in block]
    out = []
    for i in range(max(len(p) for p in per)):
        out += [p[i] for p in per if i < len(p)]
    return out


# ---- expected values ----

_hashes = {}


def window_hashes(oracle, mlen, w):
    """The oracle's hashes of the window: one run per (message, window), shared, read-only."""
    key = (mlen, w.name)
    if key not in _hashes:
        h = oracle.hash_range(MESSAGES[mlen], w.lo, w.hi - w.lo + 1)
        h.setflags(write=False)
        _hashes[key] = h
    return _hashes[key]


def range_hashes(oracle, mlen, w, a, b):
    return window_hashes(oracle, mlen, w)[a - w.lo:b - w.lo + 1]


def argmin(h, a):
    i = int(np.argmin(h))  # the first index among equal values: the lowest nonce
    return int(h[i]), a + i


def quantile(h, k):
    """The hash at the 1/k quantile of h."""
    return int(np.sort(h)[len(h) // k])


def first_targets(h):
    """(target, answer kind) x 3 of a first-hit search: the least hash (numpy's first argmin), the
    least minus 1 (nothing) and the 1/64 quantile (first_index)."""
    least = int(h.min())
    return [least, least - 1, quantile(h, 64)]


def min_jobs(oracle, named):
    """([(message, lower, upper)], [(hash, nonce)]) of block_jobs' jobs."""
    jobs, want = [], []
    for mlen, w, a, b in named:
        jobs.append((MESSAGES[mlen], a, b))
        want.append(argmin(range_hashes(oracle, mlen, w, a, b), a))
    return jobs, want


def first_jobs(oracle, named):
    """([(message, lower, upper, target)], [(hash, nonce) or None]): job k takes the (k mod 5)-th
    of its own five targets (first_batch_jobs.target_of)."""
    jobs, want = [], []
    for k, (mlen, w, a, b) in enumerate(named):
        h = range_hashes(oracle, mlen, w, a, b)
        t = target_of(h, k % KINDS)
        jobs.append((MESSAGES[mlen], a, b, t))
        want.append(first_index(h, a, t))
    return jobs, want


def collect_jobs(oracle, named):
    """([(message, lower, upper, target, cap)], [(total, hits)]): job k takes the (k mod 5)-th of
    its own five targets (collect_batch_jobs.own_targets) and the room CAPS[k mod 3]."""
    jobs, want = [], []
    for k, (mlen, w, a, b) in enumerate(named):
        h = range_hashes(oracle, mlen, w, a, b)
        t, cap = own_targets(h)[k % 5], CAPS[k % 3]
        jobs.append((MESSAGES[mlen], a, b, t, cap))
        want.append(answer(h, a, t, cap))
    return jobs, want
