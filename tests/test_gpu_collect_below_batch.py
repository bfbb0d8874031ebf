"""GPU: gpuhash_collect_below_batch -- many independent hit collections in one call, one scan
launch per kernel variant among them, each job counted and listed exactly as gpuhash_collect_below
counts and lists it.

Expected values come from the oracle (tests/collect_batch_jobs.py: oracle.hash_range + numpy); the
engine is only ever compared WITH them, and with its own Engine.collect_below on the same job.
"""
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np
import pytest

import batch_jobs
import collect_batch_jobs
from collect_batch_jobs import answer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bitcoin-miner_amd", "lib", "gpuhash_cli")
U64 = (1 << 64) - 1
AUTO = 0
COLLECT_MAX = 1 << 20
M120 = (b"The quick brown fox jumps over the lazy dog. " * 3)[:120]


@pytest.fixture(scope="module")
def mix(oracle):
    return collect_batch_jobs.jobs_and_answers(oracle)


def variants(recs):
    return {(r["shard"], r["J"], r["C2"], r["EX"]) for r in recs}


def spans(jobs):
    return sum(j[2] - j[1] + 1 for j in jobs)


# ---- 1. parity ----

@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_parity_with_the_oracle_and_with_collect_below(engine, mix, policy, rchunk):
    jobs, want = mix
    engine.set_layout_policy(policy)
    try:
        got = engine.collect_below_batch(jobs, rchunk)
        st, recs = engine.stats(), engine.launches()
        single = [engine.collect_below(m, a, b, t, cap, rchunk) for m, a, b, t, cap in jobs]
    finally:
        engine.set_layout_policy(AUTO)
    bad = [(k, jobs[k][1:], g[0], w[0]) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert got == single
    assert st["nonces"] == spans(jobs)
    assert st["launches"] == len(recs) == len(variants(recs))  # one per variant: nothing was re-run
    assert all((r["lo"], r["hi"]) == (0, len(jobs) - 1) for r in recs)  # batch records: job indices


# ---- 2. edges ----

def test_spec_example_and_the_top_of_u64(engine, oracle):
    # p1.pdf p.12: Hash("msg", 0..2) = 13781283048668101583, 4754799531757243342, 5611725180048225792
    jobs = [(b"msg", 0, 2, 5611725180048225792), (b"msg", 0, 2, U64, 1), (b"msg", 0, 2, 4754799531757243341),
            (b"msg", 0, 2, 4754799531757243342, 0)]
    assert engine.collect_below_batch(jobs) == [(2, [(4754799531757243342, 1), (5611725180048225792, 2)]),
                                                (3, [(13781283048668101583, 0)]), (0, []), (1, [])]
    assert engine.stats()["nonces"] == 12
    assert engine.count_below_batch([j[:4] for j in jobs]) == [2, 3, 0, 1]
    top = oracle.hash(b"bradfitz", U64)
    assert engine.collect_below_batch([(b"bradfitz", U64, U64, top), (b"bradfitz", U64, U64, top - 1)]) == \
        [(1, [(top, U64)]), (0, [])]
    assert engine.stats()["nonces"] == 2


def test_untouched_entries_and_the_pure_count_through_the_abi(engine):
    import gpuhash
    c = gpuhash.ctypes
    f = engine._lib.gpuhash_collect_below_batch
    buf = c.create_string_buffer(b"msgmsgmsg")
    off = (c.c_size_t * 4)(0, 3, 6, 9)
    lo, hi = (c.c_uint64 * 3)(0, 0, 0), (c.c_uint64 * 3)(2, 2, 2)
    tg = (c.c_uint64 * 3)(5611725180048225792, U64, 0)
    out_off = (c.c_size_t * 4)(0, 3, 5, 7)  # room for 3, 2 and 2: totals 2, 3 and 0
    nonces, hashes, totals = (c.c_uint64 * 7)(*[7] * 7), (c.c_uint64 * 7)(*[7] * 7), (c.c_uint64 * 3)(7, 7, 7)
    assert f(engine._ctx, c.addressof(buf), off, 3, lo, hi, tg, out_off, nonces, hashes, totals) == 0
    assert list(totals) == [2, 3, 0]
    assert list(nonces) == [1, 2, 7, 0, 1, 7, 7]
    assert list(hashes) == [4754799531757243342, 5611725180048225792, 7, 13781283048668101583, 4754799531757243342, 7, 7]
    totals = (c.c_uint64 * 3)(7, 7, 7)
    assert f(engine._ctx, c.addressof(buf), off, 3, lo, hi, tg, None, None, None, totals) == 0  # a pure count
    assert list(totals) == [2, 3, 0] and engine.stats()["nonces"] == 9


def test_4096_single_nonce_jobs(engine, oracle):
    rng = random.Random("min-batch single nonces")  # test_gpu_min_batch.py's generator
    msgs = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 8, 42, 55, 61, 64, 120)))) for _ in range(64)]
    jobs, want = [], []
    for k in range(4096):
        n = rng.randrange(10 ** rng.randrange(0, 20)) if k % 7 else U64 - rng.randrange(3)
        h = oracle.hash(msgs[k % 64], n)
        jobs.append((msgs[k % 64], n, n, h - (k & 1), 2))  # the nonce's own hash, or that minus 1
        want.append((0, []) if k & 1 else (1, [(h, n)]))
    assert engine.collect_below_batch(jobs) == want
    st, recs = engine.stats(), engine.launches()
    assert st["nonces"] == 4096 and st["launches"] == len(recs) == len(variants(recs))


# ---- 3. the device list overflows ----

def test_device_list_overflow(mix, monkeypatch):
    """GPUHASH_COLLECT_BUFFER=64: the mix's 2^64-1 jobs alone hold thousands of hits, so the shared
    list fills up, the jobs it cut short are run again alone, and every answer is still exact."""
    import gpuhash
    jobs, want = mix
    monkeypatch.setenv("GPUHASH_COLLECT_BUFFER", "64")
    with gpuhash.Engine([0]) as one:
        assert one.collect_below_batch(jobs) == want
        st, recs = one.stats(), one.launches()
    assert st["nonces"] == spans(jobs) and st["launches"] == len(recs)
    again = sorted({r["lo"] for r in recs if r["lo"] == r["hi"]})
    assert again and all((r["lo"], r["hi"]) == (0, len(jobs) - 1) for r in recs if r["lo"] != r["hi"])
    # a re-run job lists, and either holds more hits than the list or shared the run with one that does
    crowded = any(w[0] > 64 for j, w in zip(jobs, want) if j[4])
    assert all(jobs[k][4] > 0 and (want[k][0] > 64 or crowded) for k in again)
    assert {k for k, (j, w) in enumerate(zip(jobs, want)) if j[4] and w[0] > 64} <= set(again)


# ---- 4. a large job among small ones ----

def test_a_large_job_among_small_ones_keeps_its_own_counter_and_target(engine, oracle):
    import gpuhash
    big = (b"bradfitz", 0, (1 << 28) - 1, 1 << 40)  # about 16 hits
    rng = random.Random("first-below-batch large among small")  # test_gpu_first_below_batch.py's jobs
    small, want = [], []
    for k in range(100):
        lo = rng.randrange(10 ** rng.randrange(1, 12))
        m, cnt = b"other-%d" % k, rng.randrange(2, 3000)
        h = oracle.hash_range(m, lo, cnt)
        t = int(sorted(h.tolist())[cnt // 2])  # its own median hash
        small.append((m, lo, lo + cnt - 1, t, 3000))
        want.append(answer(h, lo, t, 3000))
    got = engine.collect_below_batch(small[:50] + [big] + small[50:])
    total, hits = got[50]
    assert (total, hits) == engine.collect_below(*big) and 2 <= total <= 48  # 16 expected, +-8 sigma
    assert [n for _, n in hits] == sorted({n for _, n in hits}) and len(hits) == total
    assert all(gpuhash.Hash(big[0], n) == h <= big[3] and n <= big[2] for h, n in hits)
    # a shared counter would give the small jobs the wrong totals, a shared target the wrong hits
    assert got[:50] + got[51:] == want and all(w[0] >= 1 for w in want)


# ---- 5. several context entries ----

def test_three_entries_give_the_same_results(mix):
    import gpuhash
    jobs, want = mix
    with gpuhash.Engine([0, 0, 0]) as eng:
        assert eng.collect_below_batch(jobs) == want
        recs, st = eng.launches(), eng.stats()
        assert {r["shard"] for r in recs} == {0, 1, 2} and st["ndevices"] == 3
        runs = sorted({(r["lo"], r["hi"]) for r in recs})  # contiguous runs of whole jobs covering the batch
        assert runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1 and len(runs) == 3
        assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))
        assert st["launches"] == len(recs) == len(variants(recs)) and st["nonces"] == spans(jobs)


# ---- 6. sub-batches ----

CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import hash_oracle, collect_batch_jobs, gpuhash
jobs, _ = collect_batch_jobs.jobs_and_answers(hash_oracle.load_c_oracle())
with gpuhash.Engine([0]) as eng:
    got = eng.collect_below_batch(jobs)
    print(json.dumps({{"got": got, "runs": sorted({{(r["lo"], r["hi"]) for r in eng.launches()}})}}))
"""


def test_sub_batches_on_the_device(mix):
    """GPUHASH_BATCH_BYTES small enough for at least three sub-batches, in a fresh child process."""
    jobs, want = mix
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "bitcoin-miner_amd"), os.path.join(ROOT, "oracle")]
    env = dict(os.environ, GPUHASH_BATCH_BYTES=str(256 * 1024))
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [(t, [tuple(x) for x in hits]) for t, hits in out["got"]] == want
    runs = [tuple(x) for x in out["runs"]]
    assert len(runs) >= 3 and runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1
    assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))


# ---- 7. dense hits ----

def test_dense_hits_on_the_tie_test_build(oracle):
    """libgpuhash_tietest.so keeps 4 bits of each hash: at the truncated target 3 << 32 a quarter of
    all nonces are hits and at 15 << 32 all of them, so the batch's ballots are full or nearly
    full, which real 64-bit hashes never reach at a sparse target."""
    import gpuhash
    if not os.path.exists(gpuhash.TIETEST_LIB_PATH):
        pytest.fail("libgpuhash_tietest.so not built (make -C bitcoin-miner_amd)")
    ranges = [(b"bradfitz", 999_990_000, 20_000), (M120, 9_999_990_000, 20_000), (b"x" * 53, 0, 20_000),
              (b"y" * 61, 999_900_000, 300_000)]  # test_gpu_collect_below.py's
    jobs, want = [], []
    for k, (m, lo, n) in enumerate(ranges):
        h = (oracle.hash_range(m, lo, n) >> np.uint64(60)) << np.uint64(32)  # as the build keeps them
        target = (3 << 32, 15 << 32)[k & 1]
        jobs.append((m, lo, lo + n - 1, target, n))
        want.append(answer(h, lo, target, n))
    assert [w[0] for w in want][1::2] == [20_000, 300_000] and all(0.2 * 20_000 < w[0] < 0.3 * 20_000 for w in want[::2])
    with gpuhash.Engine(lib_path=gpuhash.TIETEST_LIB_PATH) as tie:
        assert b"TIE-TEST" in tie._lib.gpuhash_version()
        assert tie.collect_below_batch(jobs) == want
        assert tie.collect_below_batch([j[:4] + (100,) for j in jobs], rchunk=7) == [(t, hits[:100]) for t, hits in want]
        assert tie.count_below_batch([j[:4] for j in jobs]) == [w[0] for w in want]


# ---- 8. the command-line client ----

def test_cli_batch_all_below(tmp_path, oracle):
    h = oracle.hash_range(b"bradfitz", 0, 10000)
    path = tmp_path / "jobs.txt"
    path.write_text(f"bradfitz 0 9999 {1 << 52}\n\nbradfitz 0 9999 1419516646206827\n"
                    f"msg 0 2 {U64} 1\nmsg 0 2 5611725180048225792 0\nbradfitz 0 9999 {U64} 3\n")
    out = subprocess.run([CLI, "--batch-all-below", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = []
    for total, hits in (answer(h, 0, 1 << 52, 256), (0, []), (3, [(13781283048668101583, 0)]), (2, []),
                        answer(h, 0, U64, 3)):
        want += [f"Total {total}"] + [f"Hit {hh} {nn}" for hh, nn in hits]
    assert out.stdout.splitlines() == want and want[0] == "Total 2"
    path.write_text("bradfitz 0 9999\n")
    assert subprocess.run([CLI, "--batch-all-below", str(path)], capture_output=True).returncode == 2
    path.write_text("bradfitz 0 9999 7 5 5\n")
    assert subprocess.run([CLI, "--batch-all-below", str(path)], capture_output=True).returncode == 2
    for line in ("bradfitz 10 5 7\n", f"bradfitz 0 9 7 {COLLECT_MAX + 1}\n"):
        path.write_text(line)
        out = subprocess.run([CLI, "--batch-all-below", str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 3 and "invalid argument" in out.stderr and out.stdout == ""


# ---- 9. it is worth having ----

def test_batch_takes_at_most_half_the_loop(engine, oracle):
    """1,024 work units, (b"share-%04d" % k, 0, 99_999, 2^50 - 1), about 6 shares each: one
    collect_below_batch against a loop of 1,024 Engine.collect_below calls over the same jobs, in
    this process; medians of five after a warm-up.  The loop is how this work is done without the
    batch call; the batch must take at most half its time, the project's bar for a batch call.
    (Measured on one MI355X, build 373022d5e8a94384: 25.21 ms against 168.26 ms, ratio 0.150,
    kernel_ms 22.02 in 2 launches, 6,162 hits; another session 26.29 against 176.11 ms, 0.149.
    DESIGN.md 3.13.)"""
    cap = 64
    jobs = [(b"share-%04d" % k, 0, 99_999, (1 << 50) - 1, cap) for k in range(1024)]

    def batch():
        t = time.perf_counter()
        got = engine.collect_below_batch(jobs)
        return time.perf_counter() - t, got

    def loop():
        t = time.perf_counter()
        got = [engine.collect_below(*j) for j in jobs]
        return time.perf_counter() - t, got

    got = batch()[1]
    assert loop()[1] == got  # warm-up, and both agree
    hits = sum(t for t, _ in got)
    assert 6250 - 640 <= hits <= 6250 + 640 and all(t == len(h) for t, h in got)  # 10^5 * 1024 / 2^14, +-8 sigma
    for k in range(0, 1024, 64):
        assert got[k] == answer(oracle.hash_range(jobs[k][0], 0, 100_000), 0, jobs[k][3], cap)
    tb = statistics.median(batch()[0] for _ in range(5))
    st, recs = engine.stats(), engine.launches()
    tl = statistics.median(loop()[0] for _ in range(5))
    print(f"\ncollect_below_batch {tb * 1e3:.2f} ms (kernel_ms {st['kernel_ms']:.3f}, {st['launches']} launches, "
          f"wall_ms {st['wall_ms']:.3f}, {hits} hits), loop of 1024 collect_below calls {tl * 1e3:.2f} ms, "
          f"ratio {tb / tl:.3f}")
    assert tb <= 0.5 * tl, (tb, tl)


def test_sparse_collection_costs_a_min_batch(engine):
    """64 jobs (b"sparse-%02d" % k, 0, 2^26-1, 2^30), about 0.25 hits in the whole batch: the
    collecting batch costs what min_batch costs on the same 64 ranges, whose code this feature
    does not touch.  Medians of five kernel_ms each, alternating, after a warm-up.  The bound is
    the larger of 2% and three times min_batch's own spread ((max - min) / median of its five runs)
    in this test: a spill or a lost wave of occupancy in the MODE 6 kernels costs far more.
    (Measured, build 373022d5e8a94384: collect_below_batch 126.003 ms (spread 0.03%), min_batch
    125.263 ms (spread 0.19%), ratio 1.0059; another session 126.057 against 125.404 ms, 1.0052.
    The bound was 2% both times.  DESIGN.md 3.13.)"""
    import gpuhash
    jobs = [(b"sparse-%02d" % k, 0, (1 << 26) - 1, 1 << 30, 16) for k in range(64)]
    mins = [j[:3] for j in jobs]
    got = engine.collect_below_batch(jobs)  # warm-up: code objects, buffers
    engine.min_batch(mins)
    t_collect, t_min = [], []
    for _ in range(5):
        assert engine.collect_below_batch(jobs) == got
        t_collect.append(engine.stats()["kernel_ms"])
        engine.min_batch(mins)
        t_min.append(engine.stats()["kernel_ms"])
    med_c, med_m = statistics.median(t_collect), statistics.median(t_min)
    spread_m = (max(t_min) - min(t_min)) / med_m
    spread_c = (max(t_collect) - min(t_collect)) / med_c
    bound = max(0.02, 3 * spread_m)
    print(f"\ncollect_below_batch median {med_c:.3f} ms (spread {spread_c * 100:.2f}%), min_batch median {med_m:.3f} ms "
          f"(spread {spread_m * 100:.2f}%), ratio {med_c / med_m:.4f}, bound {1 + bound:.4f}, "
          f"hits {sum(t for t, _ in got)}, build {gpuhash.build_id()}")
    # oracle-free invariants: 2^32 nonces at 2^-34 each, so a handful of hits at the very most
    assert sum(t for t, _ in got) <= 8 and all(t == len(h) for t, h in got)
    for (m, _, hi, target, _), (_, hits) in zip(jobs, got):
        assert all(gpuhash.Hash(m, n) == h <= target and n <= hi for h, n in hits)
    assert engine.stats()["nonces"] == 1 << 32
    assert med_c <= med_m * (1 + bound), (med_c, med_m, bound)
