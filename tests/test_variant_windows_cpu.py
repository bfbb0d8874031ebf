"""CPU: the ledger of tests/variant_windows.py -- every compiled scan kernel has a window, and
every window is what it claims to be.

No GPU here.  The two kernel manifests (tests/golden/kernel_manifest.txt and
kernel_manifest_collect_batch.txt, which tests/test_codegen.py and test_collect_below_batch_cpu.py
hold against the build) list the compiled k_scan<J, C2, EX, MODE>; their set must be the table's
layouts x the seven modes, so a kernel added without a window fails here, and so does a window
whose layout is no longer compiled.  Every window is planned with the CPU planner
(gpuhash_plan_all of libgpuhash_hostcheck.so) under its policy and held to conditions on the
INPUTS of tests/test_gpu_variant_matrix.py.  The three CPU replays of the batch modes then run
over the jobs cut from all the windows, under every policy of the table, against the oracle: the
planner, the stage and the mask replay for the layouts the shared job mix (tests/batch_jobs.py)
never reaches.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import variant_windows as vw
from first_batch_jobs import first_index
from test_collect_below_batch_cpu import replay as replay_collect
from test_collect_below_cpu import Info, plan
from test_first_below_batch_cpu import check_trace, replay as replay_first
from test_min_batch_cpu import replay as replay_min

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFESTS = ("kernel_manifest.txt", "kernel_manifest_collect_batch.txt")
u64, u32 = ctypes.c_uint64, ctypes.c_uint32
COLLECT_MAX = 1 << 20
ORDERS = [0, 12345]  # ascending, a shuffle


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(PKG, "lib", "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.gpuhash_plan_all.argtypes = [ctypes.c_char_p, u64, u64, u64, u32, ctypes.POINTER(Info), ctypes.c_int]
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_min_batch.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int, vp, vp, vp]
    lib.hostcheck_first_below_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int,
                                                vp, vp, vp, vp, vp]
    lib.hostcheck_collect_below_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int,
                                                  u64, vp, vp, vp, vp, vp]
    yield lib
    lib.hostcheck_set_layout_policy(vw.AUTO)


def layout(l):
    return (l.J, l.C2, l.EX)


def nonces(l):
    return (l.hi - l.lo) // l.stride + 1


# ---- 1. the table against the compiled kernels ----

def compiled_kernels():
    """{(J, C2, EX, MODE)} of the k_scan symbols of both manifests."""
    found = set()
    for name in MANIFESTS:
        for line in open(os.path.join(GOLDEN, name)).read().splitlines():
            m = re.search(r"k_scanILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE", line.split(" ", 2)[1])
            if m:
                found.add(tuple(int(g) for g in m.groups()))
    return found


def test_every_compiled_kernel_has_a_window_and_every_window_a_kernel():
    compiled = compiled_kernels()
    table = {lay + (mode,) for lay in vw.LAYOUTS for mode in vw.MODES}
    no_window, no_kernel = sorted(compiled - table), sorted(table - compiled)
    assert not no_window, f"{len(no_window)} compiled k_scan<J, C2, EX, MODE> have no window: {no_window}"
    assert not no_kernel, f"{len(no_kernel)} windows name a kernel that is not compiled: {no_kernel}"
    assert len(vw.TABLE) == len(vw.LAYOUTS) == len(set(vw.NAMES)) == 21  # one row per layout
    assert len(compiled) == 147


# ---- 2. every window is what it claims ----

@pytest.mark.parametrize("name", vw.NAMES)
def test_window_is_what_it_claims(hc, name):
    _, m, policy, lo, cnt, lay = vw.ROWS[name]
    hc.hostcheck_set_layout_policy(policy)
    p = plan(hc, m, lo, lo + cnt - 1, 0)
    shape = [(layout(l), l.d, nonces(l)) for l in p]
    assert sum(nonces(l) for l in p) == cnt <= vw.MAX_NONCES
    assert sum(nonces(l) for l in p if layout(l) == lay) >= vw.MIN_IN_LAYOUT, shape
    assert len(p) >= 2 and len({l.d for l in p}) >= 2, shape  # a digit-count boundary inside
    # Starts and ends inside a row.  A lane-table descriptor (C2 = 3) is a rectangle of whole
    # rows by construction (r_first = 0, r_last = R - 1: its R counts loop values, and its lanes
    # hold the last q digits), so its condition is on the lanes: it starts or ends inside the
    # 10^q lane values.
    first, last = p[0], p[-1]
    if first.C2 == 3:
        assert first.p_first > 0, shape
    else:
        assert first.r_first > 0, shape
    if last.C2 == 3:
        assert last.p_last < 10 ** last.q - 1, shape
    else:
        assert last.r_last < last.R - 1, shape
    # the batch jobs: at least four of more than one nonce run the row's layout
    in_layout = 0
    for mm, a, b in vw.row_jobs(vw.ROWS[name]):
        assert lo <= a <= b <= lo + cnt - 1
        in_layout += a < b and any(layout(l) == lay for l in plan(hc, mm, a, b, 0))
    assert in_layout >= 4, in_layout
    # the batch call of the matrix: with its partner's jobs, another message and at least two
    # kernel variants, so at least two launches
    other = vw.partner(vw.ROWS[name])
    assert other[1] != m
    seen = set()
    for _, mm, a, b in vw.interleaved([vw.ROWS[name], other]):
        seen |= {layout(l) for l in plan(hc, mm, a, b, 0)}
    assert lay in seen and len(seen) >= 2, seen


def test_jobs_are_the_cut_of_the_shared_mix():
    """batch_jobs.window_jobs' cut: the whole window, its halves, the overlap, single nonces, the
    digit crossing and nine short ranges; about 17 jobs per row."""
    for row in vw.TABLE:
        _, m, _, lo, cnt, _ = row
        jobs = vw.row_jobs(row)
        hi = lo + cnt - 1
        assert jobs[:4] == [(m, lo, hi), (m, lo, lo + cnt // 2), (m, lo + cnt // 2 + 1, hi),
                            (m, lo + cnt // 4, lo + 3 * cnt // 4)]
        assert 15 <= len(jobs) <= 19 and sum(a == b for _, a, b in jobs) >= 3
        p10 = 10 ** (len(str(hi)) - 1)
        assert (m, p10 - 1, p10) in jobs  # the crossing itself


def test_first_hit_targets_are_what_they_claim(oracle):
    """At the 1/64 quantile the first hit of every window is not its least hash, and the least
    hash is not at the window's first nonce: a kernel that returned the minimum, or the first
    nonce, would be caught.  On the tie-test build's 4-bit keys every window holds real ties."""
    for row in vw.TABLE:
        h = vw.window_hashes(oracle, row)
        none, least, dense = vw.first_targets(h)
        assert first_index(h, row[3], none) is None
        assert first_index(h, row[3], least)[1] == row[3] + int(np.argmin(h)) > row[3]
        assert first_index(h, row[3], dense)[0] > least, row[0]
        t = vw.truncated(h)
        assert int(t.min()) == 0 and int((t == 0).sum()) > len(h) // 32, row[0]


# ---- 3. the CPU replays over the new jobs ----

@pytest.fixture(scope="module")
def named():
    return vw.interleaved(vw.TABLE)


def bad(jobs, got, want):
    return [(k, len(jobs[k][0]), jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:3]


@pytest.mark.parametrize("policy", vw.POLICIES)
def test_min_batch_replay_matches_the_oracle(hc, oracle, named, policy):
    jobs, want = vw.min_jobs(oracle, named)
    for rchunk, order in ((0, ORDERS[0]), (7, ORDERS[1])):
        got, fill = replay_min(hc, jobs, rchunk, policy, order)
        assert not bad(jobs, got, want), (rchunk, order, bad(jobs, got, want))
        assert fill[2] == 0 and 0 < fill[0] <= fill[1] and fill[3] == 1, fill


@pytest.mark.parametrize("policy", vw.POLICIES)
def test_first_below_batch_replay_matches_the_oracle(hc, oracle, named, policy):
    jobs, want = vw.first_jobs(oracle, named)
    assert any(w is None for w in want) and sum(w is not None and w[1] != j[1] for j, w in zip(jobs, want)) >= 20
    for rchunk, order in ((0, ORDERS[0]), (7, ORDERS[1])):
        got, trace, fill = replay_first(hc, jobs, rchunk, policy, order)
        assert not bad(jobs, got, want), (rchunk, order, bad(jobs, got, want))
        assert fill[2] == 0 and 0 < fill[0] <= fill[1] and fill[3] == 1, fill
        check_trace(jobs, got, trace)


@pytest.mark.parametrize("policy", vw.POLICIES)
def test_collect_below_batch_replay_matches_the_oracle(hc, oracle, named, policy):
    jobs, want = vw.collect_jobs(oracle, named)
    assert [j[4] for j in jobs[:6]] == [0, 5, 5000, 0, 5, 5000]
    assert any(len(w[1]) == 5 < w[0] for w in want) and any(len(w[1]) == w[0] > 64 for w in want)
    for rchunk, order, buffer in ((0, ORDERS[0], COLLECT_MAX), (7, ORDERS[1], 64)):
        got, info = replay_collect(hc, jobs, rchunk, policy, order, buffer=buffer)
        assert not bad(jobs, got, want), (rchunk, order, buffer, bad(jobs, got, want))
        assert info[0] <= buffer and info[2] == 1, info
        assert (info[1] > 0) == (buffer == 64), info  # the short list overflows and jobs are re-run


def test_replayed_jobs_reach_every_layout(hc, named):
    """Under the table's policies the jobs of more than one nonce plan to all 21 layouts."""
    seen = set()
    for policy in vw.POLICIES:
        hc.hostcheck_set_layout_policy(policy)
        for _, m, a, b in named:
            if a < b:
                seen |= {layout(l) for l in plan(hc, m, a, b, 0)}
    assert seen >= vw.LAYOUTS, sorted(vw.LAYOUTS - seen)
