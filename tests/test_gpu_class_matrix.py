"""GPU: the scan kernels at every (message length mod 64, digit count) class, in all seven modes,
against the oracle: the windows of tests/class_windows.py, 7,952 (message, window, policy run)
cases, cut into 68 parts (class_windows.parts_of) x 7 modes = 476 test cases.  A part is a block
of 16 message lengths under the AUTO | TAIL_NEVER, AUTO | TAIL_ALWAYS and LANETABLE runs, or half
of one message length's cases under the UNIFORM run: forced on a window of 600
nonces, the two-word loop walks a row of 10^7 or 10^8 masked loop values, 17 or 170 ms per call
where the other runs take 70 us ("The class matrix", has every case's measured time).

Every call sets its policy run's layout policy (AUTO again afterwards).  After every call on one
range the set of (J, C2, EX, digits) in Engine.launches() must equal what the planner
(libgpuhash_hostcheck.so) names for that range under that policy -- per device run, should the
engine have cut the range over several devices -- and only then is the answer compared.  After a
batch call the layouts in launches() must contain every layout the planner names for the jobs.
Expected values come from one oracle.hash_range per (message, window) and numpy; the engine is
compared with them bit for bit, never with itself, except that a min-batch answer must also equal
the single call's on the first 64 jobs.  A failure names the class, the message length, the window
and the policy run.

What each mode can show.  dump (hash_range) and collect (collect_below with target 2^64-1 and room
for the whole window) return the hash of EVERY nonce of every case: they carry the per-nonce
claim, for the MODE 1 and MODE 3 kernels.  A min call reveals the hash of one nonce, the least; it
is run on every window, its halves and, for the D and E windows, each of their 16 pieces, which
raises the chance of seeing a fault that hits only some loop values and does not make it certain.
first_below examines every nonce up to its answer (all of them when nothing qualifies) but reveals
one hash as well.  The batch modes run the same ranges as jobs of one call per part and policy
run, about 8,000 jobs per block under AUTO | TAIL_NEVER, the 16 messages in turn; a UNIFORM call
holds one message's jobs, since a batch costs the sum of its jobs' row-iterations.

tests/test_class_windows_cpu.py holds the table against the planner, the kernel manifests and the
CPU replay without a GPU.
"""
import numpy as np
import pytest

import class_windows as cw
from collect_batch_jobs import answer
from first_batch_jobs import first_index

pytestmark = pytest.mark.gpu

AUTO = 0


@pytest.fixture(scope="module")
def hc():
    lib = cw.load_planner()
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


@pytest.fixture
def policy_of(request):
    """Sets an engine's layout policy for the test, AUTO again afterwards."""
    def set_policy(eng, policy):
        request.addfinalizer(lambda: eng.set_layout_policy(AUTO))
        eng.set_layout_policy(policy)
    return set_policy


def where(mlen, w, run, a, b, nonce=None):
    classes = sorted({cw.class_of(mlen, n) for n in ((a, b) if nonce is None else (nonce,))})
    at = "" if nonce is None else f", first bad nonce {nonce}"
    return (f"class (length mod 64, digits) {classes}: message length {mlen}, window {w.name}, "
            f"range [{a}, {b}], policy run {run}{at}")


def assert_launched(eng, hc, mlen, w, run, a, b):
    """The call on [a, b] ran exactly the kernel variants, at the digit counts, that the planner
    names: per device run of the call, whose ranges must cover [a, b]."""
    recs = eng.launches()
    runs = sorted({(r["lo"], r["hi"]) for r in recs})
    assert runs and runs[0][0] == a and max(hi for _, hi in runs) == b, (where(mlen, w, run, a, b), runs)
    reach = a
    for lo, hi in runs:
        assert a <= lo <= reach and hi <= b, (where(mlen, w, run, a, b), runs)
        reach = max(reach, hi + 1)
    want = set()
    for lo, hi in runs:
        want |= cw.variant_groups(cw.plan(hc, cw.MESSAGES[mlen], lo, hi, cw.POLICY[run]))
    got = {(r["J"], r["C2"], r["EX"], r["digits"]) for r in recs}
    assert got == want, (where(mlen, w, run, a, b), sorted(got), sorted(want))


def each_case(eng, hc, policy_of, part):
    """(message length, window, policy run) of the part, one policy run after the other."""
    lengths, runs, share = part
    for run in runs:
        policy_of(eng, cw.POLICY[run])
        for mlen in lengths:
            for w in cw.part_cases(hc, mlen, run, share):
                yield mlen, w, run


# ---- the single calls ----

def check_dump(eng, hc, oracle, policy_of, part):
    for mlen, w, run in each_case(eng, hc, policy_of, part):
        got = eng.hash_range(cw.MESSAGES[mlen], w.lo, w.hi - w.lo + 1)
        assert_launched(eng, hc, mlen, w, run, w.lo, w.hi)
        wrong = np.nonzero(got != cw.window_hashes(oracle, mlen, w))[0]
        assert wrong.size == 0, (where(mlen, w, run, w.lo, w.hi, w.lo + int(wrong[0])), int(wrong.size))


def check_collect(eng, hc, oracle, policy_of, part):
    for mlen, w, run in each_case(eng, hc, policy_of, part):
        m, cnt = cw.MESSAGES[mlen], w.hi - w.lo + 1
        h = cw.window_hashes(oracle, mlen, w)
        # every nonce of the window, ascending, with the oracle's hash
        total, hits = eng.collect_below(m, w.lo, w.hi, cw.U64, cnt)
        assert_launched(eng, hc, mlen, w, run, w.lo, w.hi)
        want = answer(h, w.lo, cw.U64, cnt)
        if (total, hits) != want:
            bad = next((i for i, (g, x) in enumerate(zip(hits, want[1])) if g != x), min(len(hits), cnt))
            assert False, (where(mlen, w, run, w.lo, w.hi, w.lo + bad), total, len(hits), hits[bad:bad + 1], want[1][bad:bad + 1])
        # one nonce in 16: the exact total, and the lowest five hits
        target = cw.quantile(h, 16)
        for cap in (0, 5):
            got = eng.collect_below(m, w.lo, w.hi, target, cap)
            assert_launched(eng, hc, mlen, w, run, w.lo, w.hi)
            want = answer(h, w.lo, target, cap)
            assert want[0] > cnt // 16 and len(want[1]) == cap
            assert got == want, (where(mlen, w, run, w.lo, w.hi), target, cap, got, want)


def min_ranges(w):
    """The window and its halves, and for a D or E window each of its 16 pieces."""
    return [(w.lo, w.hi)] + cw.halves(w) + (cw.pieces(w) if w.kind in "DE" else [])


def check_min(eng, hc, oracle, policy_of, part):
    for mlen, w, run in each_case(eng, hc, policy_of, part):
        for a, b in min_ranges(w):
            got = eng.min(cw.MESSAGES[mlen], a, b)
            assert_launched(eng, hc, mlen, w, run, a, b)
            want = cw.argmin(cw.range_hashes(oracle, mlen, w, a, b), a)
            # one wrong hash anywhere in the range can move the answer: the range's classes are named
            assert got == want, (where(mlen, w, run, a, b), got, want)


def check_first(eng, hc, oracle, policy_of, part):
    for mlen, w, run in each_case(eng, hc, policy_of, part):
        m, h = cw.MESSAGES[mlen], cw.window_hashes(oracle, mlen, w)
        least, none, dense = cw.first_targets(h)
        assert none >= 0
        want = (cw.argmin(h, w.lo), None, first_index(h, w.lo, dense))
        assert want[2][1] <= want[0][1]
        for target, x in zip((least, none, dense), want):
            got = eng.first_below(m, w.lo, w.hi, target)
            assert_launched(eng, hc, mlen, w, run, w.lo, w.hi)
            assert got == x, (where(mlen, w, run, w.lo, w.hi), target, got, x)


# ---- the batch calls ----

def each_batch(eng, hc, policy_of, part):
    """(policy run, jobs as class_windows.block_jobs names them) of the part.  A policy run
    without a case in the part makes no call: LANETABLE plans differently only where a J = 1
    layout straddles two blocks, at message lengths 48..62 mod 64."""
    lengths, runs, share = part
    for run in runs:
        named = cw.block_jobs(hc, lengths, run, share)
        assert named or run == "lanetable", run
        if not named:
            continue
        policy_of(eng, cw.POLICY[run])
        yield run, named


def assert_batch_launched(eng, hc, run, named):
    """Every layout the planner names for a job of the call is among the call's launches."""
    want = set()
    for mlen, _, a, b in named:
        assert a < b
        want |= {cw.layout(l) for l in cw.plan(hc, cw.MESSAGES[mlen], a, b, cw.POLICY[run])}
    got = {(r["J"], r["C2"], r["EX"]) for r in eng.launches()}
    assert got >= want, (run, sorted(want - got))


def assert_jobs(run, named, got, want):
    assert len(got) == len(want) == len(named)
    bad = [k for k, (g, x) in enumerate(zip(got, want)) if g != x]
    if bad:
        k = bad[0]
        mlen, w, a, b = named[k]
        assert False, (f"{len(bad)} jobs differ, the first is job {k}", where(mlen, w, run, a, b), got[k], want[k])


def check_min_batch(eng, hc, oracle, policy_of, part):
    for run, named in each_batch(eng, hc, policy_of, part):
        jobs, want = cw.min_jobs(oracle, named)
        got = eng.min_batch(jobs)
        assert_batch_launched(eng, hc, run, named)
        assert_jobs(run, named, got, want)
        assert got[:64] == [eng.min(*j) for j in jobs[:64]]


def check_first_batch(eng, hc, oracle, policy_of, part):
    for run, named in each_batch(eng, hc, policy_of, part):
        jobs, want = cw.first_jobs(oracle, named)
        got = eng.first_below_batch(jobs)
        assert_batch_launched(eng, hc, run, named)
        assert_jobs(run, named, got, want)


def check_collect_batch(eng, hc, oracle, policy_of, part):
    for run, named in each_batch(eng, hc, policy_of, part):
        jobs, want = cw.collect_jobs(oracle, named)
        got = eng.collect_below_batch(jobs)
        assert_batch_launched(eng, hc, run, named)
        assert_jobs(run, named, got, want)


CHECKS = (check_min, check_dump, check_first, check_collect, check_min_batch, check_first_batch, check_collect_batch)


@pytest.mark.parametrize("part,mode", [c[1:] for c in cw.GPU_CASES],
                         ids=[f"{name}-{cw.MODES[mode]}" for name, _, mode in cw.GPU_CASES])
def test_class_matrix(engine, hc, oracle, policy_of, part, mode):
    CHECKS[mode](engine, hc, oracle, policy_of, part)
