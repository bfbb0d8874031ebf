"""GPU: gpuhash_first_below_batch_early -- gpuhash_first_below_batch's answers, with the front of
every job hashed packed by k_pack_first in ascending rounds of doubling pieces.

Expected values come from the oracle (tests/packed_jobs.py, tests/first_batch_jobs.py:
oracle.hash_range + the first index at or below the target) and from the committed fixture
tests/golden/first_below_batch.json; the engine is only ever compared WITH them, and with its own
Engine.first_below_batch on the same jobs.
"""
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import pytest

import batch_jobs
import first_batch_jobs
import packed_jobs
from first_batch_jobs import first_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
CLI = os.path.join(PKG, "lib", "gpuhash_cli")
PATHS = [os.path.join(ROOT, "tests"), PKG, os.path.join(ROOT, "oracle")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "first_below_batch.json")
U64 = (1 << 64) - 1
AUTO = 0
ECANCELED = -6
ROUND_ITEMS = 1 << 20
BOUNDARY_LOWERS = [95, 9990, 99999990, 10 ** 19 - 100, (1 << 64) - 5001]


@pytest.fixture(scope="module")
def one():
    """One context entry on device 0: `a launch per round` means the same on any machine."""
    import gpuhash
    e = gpuhash.Engine([0])
    yield e
    e.close()


@pytest.fixture(scope="module")
def mix(oracle):
    return first_batch_jobs.jobs_and_answers(oracle)


@pytest.fixture(scope="module")
def boundary(oracle):
    """The digit-boundary jobs of tests/test_first_below_early_cpu.py: the target is the least hash
    from offset 3000 on."""
    jobs, want = [], []
    for i, lo in enumerate(BOUNDARY_LOWERS):
        m = b"early-%d" % i + b"z" * (11 * i)
        hi = min(lo + 5000, U64)
        h = oracle.hash_range(m, lo, hi - lo + 1)
        t = int(h[3000:].min())
        jobs.append((m, lo, hi, t))
        want.append(first_index(h, lo, t))
    return jobs, want


@pytest.fixture(scope="module")
def stamps():
    with open(GOLDEN) as f:
        g = json.load(f)
    jobs = [(bytes.fromhex(j["msg_hex"]), g["lower"], g["upper"], g["target"]) for j in g["jobs"]]
    return jobs, [(j["hash"], j["nonce"]) for j in g["jobs"]]


def first_chunk(fronts):
    c = 64
    while c < ROUND_ITEMS and c * fronts < ROUND_ITEMS:
        c *= 2
    return c


def limit_of(lo, hi, target, prefix=0):
    import gpuhash
    span = hi - lo + 1
    if prefix:
        return min(span, prefix)
    e = -((-(1 << 64)) // (target + 1))
    return min(span, 4 * e) if 4 * e <= gpuhash.EARLY_MAX_PREFIX else 0


def packed_records(recs):
    return [r for r in recs if r["C2"] == 4]


def packed_come_first(recs):
    kinds = [r["C2"] == 4 for r in recs]
    return kinds == sorted(kinds, reverse=True) and all(
        (r["J"], r["EX"], r["digits"]) == (-1, 0, 0) and r["c"] in (1, 2) for r in packed_records(recs))


def digits_never_decrease(recs):
    runs = {}
    for r in recs:
        runs.setdefault((r["shard"], r["lo"], r["hi"]), []).append(r["digits"])
    return all(d == sorted(d) for d in runs.values())


# ---- 1. the class matrix ----

def test_class_matrix_all_packed(one, oracle, boundary):
    """Every (length mod 64, digit count) class, both tail block counts, a 2^20-byte message and
    the top of uint64, with the five kinds of target; prefix 2^20 covers every span."""
    jobs3 = packed_jobs.matrix()
    hs = packed_jobs.hashes(oracle, jobs3)
    jobs, want = [], []
    for k, ((m, a, b), h) in enumerate(zip(jobs3, hs)):
        t = first_batch_jobs.target_of(h, k % first_batch_jobs.KINDS)
        jobs.append((m, a, b, t))
        want.append(first_index(h, a, t))
    jobs, want = jobs + boundary[0], want + boundary[1]
    got = one.first_below_batch_early(jobs, prefix=1 << 20)
    bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    st, recs = one.stats(), one.launches()
    assert recs and all(r["C2"] == 4 for r in recs) and packed_come_first(recs)
    assert st["launches"] == len(recs) >= 2  # the boundary jobs' 5001 nonces: rounds of 1024, 2048, 4096
    assert recs[0]["c"] == 2 and recs[0]["nonces"] == 5 * len(jobs3) - 72 + 5 * 1024  # [0, 3] has 4 nonces
    assert st["nonces"] == first_batch_jobs.examined(jobs, want)


# ---- 2. the mix ----

@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_the_mix_under_every_policy(one, mix, policy, rchunk):
    jobs, want = mix
    one.set_layout_policy(policy)
    try:
        plain = one.first_below_batch(jobs, rchunk)
        for prefix in (0, 1, 1000, 1 << 20):
            got = one.first_below_batch_early(jobs, prefix, rchunk)
            bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad, (prefix, bad[:3])
            assert got == plain
            st, recs = one.stats(), one.launches()
            assert st["nonces"] == first_batch_jobs.examined(jobs, want)
            assert st["launches"] == len(recs) and packed_come_first(recs)
            assert (len(packed_records(recs)) == len(recs)) == (prefix == 1 << 20)
    finally:
        one.set_layout_policy(AUTO)


# ---- 3. the golden's 256 stamps ----

def test_the_stamps_run_both_phases(one, stamps):
    jobs, want = stamps
    assert one.first_below_batch_early(jobs) == want
    st, recs = one.stats(), one.launches()
    limit = limit_of(*jobs[0][1:])
    c0 = first_chunk(len(jobs))
    assert limit == 1 << 18 and c0 == 4096
    assert max(w[1] for w in want) > limit  # some answers lie beyond the front: both phases run
    packed, rest = packed_records(recs), [r for r in recs if r["C2"] != 4]
    assert packed and rest and packed_come_first(recs) and st["launches"] == len(recs)
    assert sum(r["nonces"] for r in packed) <= sum(min(limit, 2 * w[1] + c0) for w in want)
    assert [r["nonces"] for r in packed][0] == c0 * len(jobs)
    assert all(0 <= r["lo"] <= r["hi"] < len(jobs) for r in recs)
    assert digits_never_decrease(rest), [r["digits"] for r in rest]
    beyond = [k for k, w in enumerate(want) if w[1] >= limit]
    assert all((r["lo"], r["hi"]) == (beyond[0], beyond[-1]) for r in rest)
    assert st["nonces"] == sum(w[1] + 1 for w in want)


# ---- 4. digit boundaries ----

def test_digit_boundaries_inside_a_chunk_and_between_rounds(one, boundary):
    jobs, want = boundary
    for prefix in (0, 1000, 1 << 20):
        assert one.first_below_batch_early(jobs, prefix) == want, prefix
    # beside 1,100 two-nonce jobs c_0 is 1024: the answers lie in the second or third round
    filler = [(b"f%d" % k, 98 + k % 3, 99 + k % 3, U64) for k in range(1100)]
    got = one.first_below_batch_early(jobs + filler, 1 << 20)
    assert got[:5] == want and all(g is not None and g[1] == f[1] for g, f in zip(got[5:], filler))
    recs = one.launches()
    assert [r["nonces"] for r in recs][0] == 5 * 1024 + 2 * 1100 and len(recs) >= 2 and all(r["C2"] == 4 for r in recs)


# ---- 5. a scan-only job among stamps ----

def test_a_scan_only_job_among_stamps(one, stamps):
    jobs = list(stamps[0][:63])
    jobs.insert(31, (b"scan-only", 0, (1 << 26) - 1, 0))
    got = one.first_below_batch_early(jobs)
    recs = one.launches()
    assert got[31] is None and got[:31] + got[32:] == stamps[1][:63]
    packed = packed_records(recs)
    assert packed and not [r for r in packed if r["lo"] == r["hi"] == 31]
    assert packed[0]["nonces"] == 63 * first_chunk(63)  # 63 fronts, not 64
    assert got == one.first_below_batch(jobs)


# ---- 6. several entries and sub-batches ----

def test_three_entries_give_the_same_results(mix, stamps):
    import gpuhash
    with gpuhash.Engine([0, 0, 0]) as eng:
        for prefix in (0, 1000, 1 << 20):
            assert eng.first_below_batch_early(mix[0], prefix) == mix[1]
            recs = eng.launches()
            assert {r["shard"] for r in packed_records(recs)} == {0, 1, 2} and eng.stats()["launches"] == len(recs)
        assert eng.first_below_batch_early(stamps[0]) == stamps[1]
        assert eng.stats()["ndevices"] == 3


CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import first_batch_jobs, gpuhash, hash_oracle
jobs, _ = first_batch_jobs.jobs_and_answers(hash_oracle.load_c_oracle())
with gpuhash.Engine([0]) as eng:
    out = {{"mix": eng.first_below_batch_early(jobs, 1 << 20)}}
    out["recs"] = [(r["C2"], r["lo"], r["hi"]) for r in eng.launches()]
    out["rule"] = eng.first_below_batch_early(jobs)
    print(json.dumps(out))
"""


def test_sub_batches_on_the_device(mix):
    """GPUHASH_BATCH_BYTES = 16 KiB in a fresh child process cuts every round of the mix into
    several sub-batches, each a launch of its own."""
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=PATHS)],
                       env=dict(os.environ, GPUHASH_BATCH_BYTES=str(16 * 1024)), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    want = [list(w) if w else None for w in mix[1]]
    assert out["mix"] == want and out["rule"] == want
    runs = sorted({(lo, hi) for c2, lo, hi in out["recs"]})
    assert all(c2 == 4 for c2, _, _ in out["recs"]) and len(runs) >= 3
    assert runs[0][0] == 0 and runs[-1][1] == len(mix[0]) - 1


# ---- 7. cancel ----

def test_cancel_inside_the_packed_rounds(one, mix):
    """DESIGN.md 3.15's cancel workload: 4,096 jobs of 2^20 nonces, nothing qualifies, prefix 2^20,
    so every nonce is hashed packed, in thirteen rounds.  Run once left alone, then cancelled the
    first time progress() shows work handed out.  The latency condition is
    tests/test_gpu_cancel.py's: the cancelled call takes at most half of the call left alone."""
    import gpuhash
    jobs = [(b"cancel-%04d" % k, 10 ** 7, 10 ** 7 + (1 << 20) - 1, 0) for k in range(4096)]
    n, data, off, lower, upper, target = one._batch_arrays(jobs, 0, 4)
    sent = 0x5A5A5A5A5A5A5A5A
    c = gpuhash.ctypes
    out = {}

    def arrays():
        return (c.c_uint64 * n)(*[sent] * n), (c.c_uint64 * n)(*[sent] * n), (c.c_int * n)(*[77] * n)

    def call(hashes, nonces, found):
        t = time.perf_counter()
        out["rc"] = one._lib.gpuhash_first_below_batch_early(one._ctx, c.addressof(data), off, n, lower, upper, target,
                                                             1 << 20, 0, hashes, nonces, found)
        out["wall"] = time.perf_counter() - t

    hashes, nonces, found = arrays()
    call(hashes, nonces, found)
    alone = out["wall"]
    assert out["rc"] == 0 and all(v == 0 for v in found) and all(v == sent for v in hashes)
    recs = one.launches()
    assert all(r["C2"] == 4 for r in recs) and sum(r["nonces"] for r in recs) == one.stats()["nonces"] == 4096 << 20
    hashes, nonces, found = arrays()
    try:
        th = threading.Thread(target=call, args=(hashes, nonces, found))
        th.start()
        cancelled, deadline = None, time.perf_counter() + 20
        while th.is_alive() and time.perf_counter() < deadline:
            done, total = one.progress()
            if done > 0:
                cancelled = (done, total)
                one.cancel()
                break
            time.sleep(0.001)
        th.join(30)
        assert not th.is_alive(), "the call did not return"
        one.resume()
        print(f"\nalone {alone * 1e3:.1f} ms; cancelled at {cancelled}, the call took {out['wall'] * 1e3:.1f} ms")
        assert cancelled is not None and cancelled[1] == 4096 << 20 and cancelled[0] <= cancelled[1]
        assert out["rc"] == ECANCELED
        assert all(v == sent for v in hashes) and all(v == sent for v in nonces) and all(v == 77 for v in found)
        assert out["wall"] <= 0.5 * alone, (out["wall"], alone)
        assert one.first_below_batch_early(mix[0]) == mix[1]
    finally:
        one.resume()


# ---- 8. the CLI ----

def test_cli_early_prints_what_batch_below_prints(tmp_path, stamps):
    jobs, want = stamps
    lines = [f"{m.decode()} {a} {b} {t}" for m, a, b, t in jobs[:9]] + ["nothing 0 999 0"]
    path = tmp_path / "stamps.txt"
    path.write_text("\n".join(lines) + "\n")
    plain = subprocess.run([CLI, "--batch-below", str(path)], capture_output=True, text=True, timeout=120)
    early = subprocess.run([CLI, "--early", "--batch-below", str(path)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and early.returncode == 0, plain.stderr + early.stderr
    assert early.stdout == plain.stdout == "".join(f"Result {h} {n}\n" for h, n in want[:9]) + "None\n"


# ---- 9. it is worth having ----

def test_early_is_not_slower_on_the_stamps(one, stamps):
    """The 256 stamps through first_below_batch_early against first_below_batch, alternating on one
    engine in one process; medians of five wall times after a warm-up each.  The condition: the new
    call's median is not above first_below_batch's.  The figures are printed; DESIGN.md 3.16 records
    the measured ones."""
    jobs, want = stamps

    def run(early):
        t = time.perf_counter()
        got = one.first_below_batch_early(jobs) if early else one.first_below_batch(jobs)
        wall = time.perf_counter() - t
        recs = one.launches()
        return wall, got, one.stats(), sum(r["nonces"] for r in recs if r["C2"] == 4)

    assert run(True)[1] == want and run(False)[1] == want  # warm-up, and both are right
    te, tp, ke, kp = [], [], [], []
    for _ in range(5):
        t, got, st, packed = run(True)
        assert got == want
        te.append(t)
        ke.append(st["kernel_ms"])
        le = st["launches"]
        t, got, st, _ = run(False)
        assert got == want
        tp.append(t)
        kp.append(st["kernel_ms"])
        lp = st["launches"]
    me, mp = statistics.median(te), statistics.median(tp)
    print(f"\n256 stamps: early {me * 1e3:.2f} ms (kernel_ms {statistics.median(ke):.3f}, {le} launches, "
          f"{packed} packed nonces), first_below_batch {mp * 1e3:.2f} ms (kernel_ms {statistics.median(kp):.3f}, "
          f"{lp} launches), ratio {me / mp:.3f}")
    assert me <= mp, (me, mp)


# ---- 10. it costs nothing when nothing is early ----

def test_nothing_early_costs_nothing(one):
    """64 jobs of 2^26 nonces with target 0: the rule gives no job a front, so the launches are
    first_below_batch's, and the median of five is within the larger of 2% and three times
    first_below_batch's own (max - min) / median (DESIGN.md 3.9's rule)."""
    jobs = [(b"msg%d" % k, 0, (1 << 26) - 1, 0) for k in range(64)]

    def run(early):
        t = time.perf_counter()
        got = one.first_below_batch_early(jobs) if early else one.first_below_batch(jobs)
        wall = time.perf_counter() - t
        assert got == [None] * 64
        return wall, [(r["digits"], r["J"], r["C2"], r["EX"], r["lo"], r["hi"], r["nonces"]) for r in one.launches()]

    keys_e, keys_p = run(True)[1], run(False)[1]  # warm-up
    assert keys_e == keys_p and not [k for k in keys_e if k[2] == 4]
    te, tp = [], []
    for _ in range(5):
        te.append(run(True)[0])
        tp.append(run(False)[0])
    me, mp = statistics.median(te), statistics.median(tp)
    tol = max(0.02, 3 * (max(tp) - min(tp)) / mp)
    print(f"\n64 x 2^26, target 0: early {me * 1e3:.2f} ms, first_below_batch {mp * 1e3:.2f} ms, "
          f"ratio {me / mp:.4f}, tolerance {tol:.4f}")
    assert me <= mp * (1 + tol), (me, mp, tol)
