"""GPU: every compiled scan kernel k_scan<J, C2, EX, MODE> runs, and computes what the oracle
computes: 21 layouts (the rows of tests/variant_windows.py) x 7 modes, 147 cases.

Every case sets its row's layout policy (and restores AUTO afterwards), makes the call, asserts
from Engine.launches() that the row's (J, C2, EX) ran -- in the whole-window calls, on at least
1,500 nonces -- and only then compares.  Expected values come from one oracle.hash_range per
window and numpy; the engine is compared with them bit for bit, never with itself, except that a
batch answer must also equal the single-job call's on the same job.  The batch modes run the
row's jobs interleaved with another row's, so every workgroup changes job and message and the
call makes at least two launches, one per kernel variant.

The tie part runs each row through libgpuhash_tietest.so, which keeps the top 4 bits of each
hash: one nonce in 16 shares the least key and a quarter of them meet the target 3 << 32, so a
layout whose lane-to-nonce order is wrong returns a wrong but plausible nonce here.

tests/test_variant_windows_cpu.py holds the table against the kernel manifests and the planner
without a GPU.
"""
import os

import numpy as np
import pytest

import variant_windows as vw
from collect_batch_jobs import answer, own_targets
from first_batch_jobs import first_index

pytestmark = pytest.mark.gpu

AUTO = 0
MODE_NAMES = ("min", "dump", "first", "collect", "min-batch", "first-batch", "collect-batch")
TIE_HIT = 3 << 32  # a quarter of the truncated hashes are at or below it


def ran(eng, lay, at_least=1):
    """Asserts that the last call launched the layout's kernel on at least `at_least` nonces."""
    recs = eng.launches()
    mine = sum(r["nonces"] for r in recs if (r["J"], r["C2"], r["EX"]) == lay)
    assert mine >= at_least, (lay, [(r["J"], r["C2"], r["EX"], r["nonces"]) for r in recs])
    return recs


def one_launch_per_variant(eng, recs, per_digits=False):
    keys = {(r["shard"], r["J"], r["C2"], r["EX"]) + ((r["digits"],) if per_digits else ()) for r in recs}
    assert eng.stats()["launches"] == len(recs) == len(keys) >= 2, sorted(keys)


def ranges(lo, cnt):
    """The whole window, its halves and the range that overlaps both, inclusive."""
    hi, half = lo + cnt - 1, lo + cnt // 2
    return [(lo, hi), (lo, half), (half + 1, hi), (lo + cnt // 4, lo + 3 * cnt // 4)]


def argmin(h, lo, a, b):
    part = h[a - lo:b - lo + 1]
    i = int(np.argmin(part))  # the first index among equal values: the lowest nonce
    return int(part[i]), a + i


def differ(jobs, got, want):
    return [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:3]


@pytest.fixture
def policy_of(request):
    """Sets an engine's layout policy for the test, AUTO again afterwards."""
    def set_policy(eng, policy):
        request.addfinalizer(lambda: eng.set_layout_policy(AUTO))
        eng.set_layout_policy(policy)
    return set_policy


# ---- the seven modes ----

def check_min(eng, oracle, row):
    _, m, _, lo, cnt, lay = row
    h = vw.window_hashes(oracle, row)
    for rchunk in (0, 7):
        for k, (a, b) in enumerate(ranges(lo, cnt)):
            got = eng.min(m, a, b, rchunk)
            if k == 0:
                ran(eng, lay, vw.MIN_IN_LAYOUT)
            assert got == argmin(h, lo, a, b), (rchunk, a, b)


def check_dump(eng, oracle, row):
    _, m, _, lo, cnt, lay = row
    got = eng.hash_range(m, lo, cnt)
    ran(eng, lay, vw.MIN_IN_LAYOUT)
    wrong = np.nonzero(got != vw.window_hashes(oracle, row))[0]
    assert wrong.size == 0, ("first bad nonce", lo + int(wrong[0]), wrong.size)


def check_first(eng, oracle, row):
    _, m, _, lo, cnt, lay = row
    h = vw.window_hashes(oracle, row)
    none, least, dense = vw.first_targets(h)
    assert eng.first_below(m, lo, lo + cnt - 1, none) is None  # every nonce is examined
    ran(eng, lay, vw.MIN_IN_LAYOUT)
    for target in (least, dense):
        assert eng.first_below(m, lo, lo + cnt - 1, target) == first_index(h, lo, target), target


def check_collect(eng, oracle, row):
    _, m, _, lo, cnt, lay = row
    h = vw.window_hashes(oracle, row)
    for ti, target in enumerate(own_targets(h)):
        for cap in (0, 5, cnt):
            got = eng.collect_below(m, lo, lo + cnt - 1, target, cap)
            ran(eng, lay, vw.MIN_IN_LAYOUT)
            want = answer(h, lo, target, cap)
            assert ti not in (0, 1, 4) or want[0] == {0: 0, 1: 1, 4: cnt}[ti]
            assert got == want, (ti, target, cap, got[0], want[0])


def check_min_batch(eng, oracle, row):
    jobs, want = vw.min_jobs(oracle, vw.interleaved([row, vw.partner(row)]))
    got = eng.min_batch(jobs)
    one_launch_per_variant(eng, ran(eng, row[5]))
    assert not differ(jobs, got, want), differ(jobs, got, want)
    assert got == [eng.min(*j) for j in jobs]


def check_first_batch(eng, oracle, row):
    jobs, want = vw.first_jobs(oracle, vw.interleaved([row, vw.partner(row)]))
    got = eng.first_below_batch(jobs)
    one_launch_per_variant(eng, ran(eng, row[5]), per_digits=True)
    assert not differ(jobs, got, want), differ(jobs, got, want)
    assert got == [eng.first_below(*j) for j in jobs]


def check_collect_batch(eng, oracle, row):
    jobs, want = vw.collect_jobs(oracle, vw.interleaved([row, vw.partner(row)]))
    got = eng.collect_below_batch(jobs)
    one_launch_per_variant(eng, ran(eng, row[5]))
    assert not differ(jobs, got, want), differ(jobs, got, want)
    assert got == [eng.collect_below(*j) for j in jobs]


CHECKS = (check_min, check_dump, check_first, check_collect, check_min_batch, check_first_batch, check_collect_batch)


@pytest.mark.parametrize("mode", vw.MODES, ids=MODE_NAMES)
@pytest.mark.parametrize("name", vw.NAMES)
def test_kernel_matches_the_oracle(engine, oracle, policy_of, name, mode):
    row = vw.ROWS[name]
    policy_of(engine, row[2])
    CHECKS[mode](engine, oracle, row)


# ---- ties ----

@pytest.fixture(scope="module")
def tie_engine():
    import gpuhash
    if not os.path.exists(gpuhash.TIETEST_LIB_PATH):
        pytest.fail("libgpuhash_tietest.so not built (make -C bitcoin-miner_amd)")
    eng = gpuhash.Engine(lib_path=gpuhash.TIETEST_LIB_PATH)
    assert b"TIE-TEST" in eng._lib.gpuhash_version()
    yield eng
    eng.close()


@pytest.mark.parametrize("name", vw.NAMES)
def test_lowest_nonce_and_dense_hits_on_the_tie_test_build(tie_engine, oracle, policy_of, name):
    row = vw.ROWS[name]
    _, m, policy, lo, cnt, lay = row
    hi = lo + cnt - 1
    h = vw.truncated(vw.window_hashes(oracle, row))
    assert int(h.min()) == 0 and (h == 0).sum() > cnt // 32  # real ties for the least key
    policy_of(tie_engine, policy)
    named = vw.interleaved([row, vw.partner(row)])
    # min and min_batch: the lowest nonce among the ties
    for rchunk in (0, 7):
        for k, (a, b) in enumerate(ranges(lo, cnt)):
            got = tie_engine.min(m, a, b, rchunk)
            if k == 0:
                ran(tie_engine, lay, vw.MIN_IN_LAYOUT)
            assert got == argmin(h, lo, a, b), (rchunk, a, b)
    jobs, want = vw.min_jobs(oracle, named, tie=True)
    got = tie_engine.min_batch(jobs)
    one_launch_per_variant(tie_engine, ran(tie_engine, lay))
    assert not differ(jobs, got, want), differ(jobs, got, want)
    # first_below at the least key, from the window's start and from inside the row's layout
    for a, b in ranges(lo, cnt):
        assert tie_engine.first_below(m, a, b, 0) == first_index(h[a - lo:b - lo + 1], a, 0), (a, b)
    # collect_below and collect_below_batch with nearly full ballots
    want_all = answer(h, lo, TIE_HIT, cnt)
    assert 0.2 * cnt < want_all[0] < 0.3 * cnt
    got = tie_engine.collect_below(m, lo, hi, TIE_HIT, cnt)
    ran(tie_engine, lay, vw.MIN_IN_LAYOUT)
    assert got == want_all
    jobs, want = vw.collect_jobs(oracle, named, tie_target=TIE_HIT)
    got = tie_engine.collect_below_batch(jobs)
    one_launch_per_variant(tie_engine, ran(tie_engine, lay))
    assert not differ(jobs, got, want), differ(jobs, got, want)
