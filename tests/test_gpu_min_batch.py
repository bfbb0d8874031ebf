"""GPU: gpuhash_min_batch -- many independent searches in one call, one scan launch per kernel
variant among them, each job answered exactly as gpuhash_min answers it.

Expected values come from the oracle (tests/batch_jobs.py: oracle.hash_range + numpy argmin,
lowest index), the large one from the golden scanner (tests/golden/min_batch.json); the engine
is only ever compared WITH them, and with its own Engine.min on the same job.
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
AUTO = 0
TINY = 1024  # jobs [0, 9999], one 8-byte message each


@pytest.fixture(scope="module")
def mix(oracle):
    named = batch_jobs.job_mix()
    return [(m, a, b) for _, m, a, b in named], batch_jobs.expected(oracle, named)


@pytest.fixture(scope="module")
def tiny(oracle):
    """1,024 config-1-sized jobs over distinct 8-byte messages, and the oracle's answers."""
    jobs = [(b"job-%04d" % k, 0, 9999) for k in range(TINY)]
    return jobs, [oracle.min(m, a, b) for m, a, b in jobs]


def variant_groups(eng):
    return {(r["J"], r["C2"], r["EX"]) for r in eng.launches()}


# ---- 1. parity ----

@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_parity_with_the_oracle_and_with_min(engine, mix, policy, rchunk):
    jobs, want = mix
    engine.set_layout_policy(policy)
    try:
        got = engine.min_batch(jobs, rchunk)
        st, groups = engine.stats(), variant_groups(engine)
        single = [engine.min(m, a, b, rchunk) for m, a, b in jobs]
    finally:
        engine.set_layout_policy(AUTO)
    bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert got == single
    assert st["launches"] == len(groups) < 32  # one launch per kernel variant, not per job
    assert st["nonces"] == sum(b - a + 1 for _, a, b in jobs)


# ---- 2. many tiny jobs ----

def test_1024_config1_sized_jobs(engine, tiny):
    jobs, want = tiny
    assert engine.min_batch(jobs) == want
    st, recs = engine.stats(), engine.launches()
    # each job plans to 4 descriptors in 2 variant groups: 2 launches for the 1,024 jobs
    assert st["launches"] == len(recs) == 2 and {(r["J"], r["C2"], r["EX"]) for r in recs} == {(2, 0, 0), (3, 0, 0)}
    assert sorted(r["nonces"] for r in recs) == [1000 * TINY, 9000 * TINY]
    assert all((r["lo"], r["hi"]) == (0, TINY - 1) for r in recs)  # batch records: job indices
    assert st["nonces"] == 10000 * TINY


def test_4096_single_nonce_jobs(engine, oracle):
    rng = random.Random("min-batch single nonces")
    msgs = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 8, 42, 55, 61, 64, 120)))) for _ in range(64)]
    jobs = []
    for k in range(4096):
        n = rng.randrange(10 ** rng.randrange(0, 20)) if k % 7 else U64 - rng.randrange(3)
        jobs.append((msgs[k % 64], n, n))
    got = engine.min_batch(jobs)
    assert got == [(oracle.hash(m, n), n) for m, n, _ in jobs]
    st = engine.stats()
    assert st["launches"] == len(variant_groups(engine)) < 32 and st["nonces"] == 4096


def test_a_span_over_the_maximum_is_refused_by_a_live_context_too(engine):
    import gpuhash
    with pytest.raises(ValueError):
        engine.min_batch([(b"x", 5, 5 + gpuhash.GPUHASH_BATCH_MAX_SPAN)])
    h, n = (gpuhash.ctypes.c_uint64 * 1)(), (gpuhash.ctypes.c_uint64 * 1)()
    off = (gpuhash.ctypes.c_size_t * 2)(0, 1)
    lo, hi = (gpuhash.ctypes.c_uint64 * 1)(5), (gpuhash.ctypes.c_uint64 * 1)(5 + gpuhash.GPUHASH_BATCH_MAX_SPAN)
    buf = gpuhash.ctypes.create_string_buffer(b"x")
    rc = engine._lib.gpuhash_min_batch(engine._ctx, gpuhash.ctypes.addressof(buf), off, 1, lo, hi, h, n)
    assert rc == gpuhash.GPUHASH_EINVAL and (h[0], n[0]) == (0, 0)


# ---- 3. per-job pruning ----

def test_a_large_job_between_small_ones_keeps_its_own_threshold(engine, oracle):
    with open(os.path.join(ROOT, "tests", "golden", "min_batch.json")) as f:
        g = {r["name"]: r for r in json.load(f)["ranges"]}["bradfitz_2p28"]
    big = (bytes.fromhex(g["msg_hex"]), g["lower"], g["upper"])
    assert big == (b"bradfitz", 0, (1 << 28) - 1) and oracle.hash(big[0], g["nonce"]) == g["hash"]
    rng = random.Random("min-batch pruning")
    small = []
    for k in range(100):
        lo = rng.randrange(10 ** rng.randrange(1, 12))
        small.append((b"other-%d" % k, lo, lo + rng.randrange(1, 3000)))
    jobs = small[:50] + [big] + small[50:]
    got = engine.min_batch(jobs)
    assert got[50] == (g["hash"], g["nonce"])
    # the small jobs' answers are far above the large job's: a shared threshold would lose them
    want = [oracle.min(m, a, b) for m, a, b in small]
    assert got[:50] + got[51:] == want and min(h for h, _ in want) > g["hash"]


# ---- 4. ties ----

def test_each_job_keeps_the_lowest_nonce_of_its_own_range():
    import gpuhash
    import hash_oracle
    oracle = hash_oracle.load_c_oracle()
    if not os.path.exists(gpuhash.TIETEST_LIB_PATH):
        pytest.fail("libgpuhash_tietest.so not built (make -C bitcoin-miner_amd)")
    m120 = (b"The quick brown fox jumps over the lazy dog. " * 3)[:120]
    jobs, want = [], []
    for m, lo in ((b"bradfitz", 999_950_000), (m120, 9_999_950_000), (b"y" * 56, 90_000)):
        # keys truncated to 4 bits: about one nonce in 16 shares the least key
        k = (oracle.hash_range(m, lo, 110_000) >> np.uint64(60)) << np.uint64(32)
        for a, b in [(j * 9_000, j * 9_000 + 30_000) for j in range(9)] + [(7, 7), (0, 109_999), (50_000, 50_063)]:
            i = int(np.argmin(k[a:b + 1]))  # first occurrence = lowest nonce
            jobs.append((m, lo + a, lo + b))
            want.append((int(k[a + i]), lo + a + i))
    order = list(range(len(jobs)))
    random.Random("min-batch ties").shuffle(order)  # interleave the messages
    with gpuhash.Engine(lib_path=gpuhash.TIETEST_LIB_PATH) as eng:
        assert b"TIE-TEST" in eng._lib.gpuhash_version()
        for rchunk in (0, 7):
            assert eng.min_batch([jobs[i] for i in order], rchunk) == [want[i] for i in order]


# ---- 5. several context entries ----

def test_three_entries_give_the_same_results(mix, tiny):
    import gpuhash
    with gpuhash.Engine([0, 0, 0]) as eng:
        for jobs, want in (mix, tiny):
            assert eng.min_batch(jobs) == want
            recs, st = eng.launches(), eng.stats()
            assert {r["shard"] for r in recs} == {0, 1, 2} and st["ndevices"] == 3
            # contiguous runs of whole jobs, in order, covering the batch
            runs = sorted({(r["lo"], r["hi"]) for r in recs})
            assert runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1 and len(runs) == 3
            assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))
            assert st["launches"] == len(recs)


# ---- 6. sub-batches ----

CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import batch_jobs, gpuhash
jobs = [(m, a, b) for _, m, a, b in batch_jobs.job_mix()]
with gpuhash.Engine([0]) as eng:
    got = eng.min_batch(jobs)
    print(json.dumps({{"got": got, "launches": eng.stats()["launches"],
                      "runs": sorted({{(r["lo"], r["hi"]) for r in eng.launches()}})}}))
"""


def test_sub_batches_on_the_device(mix):
    """GPUHASH_BATCH_BYTES small enough for at least three sub-batches, in a fresh child process
    (the engine reads it per call, but a child keeps this process's environment as it was)."""
    jobs, want = mix
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "bitcoin-miner_amd"), os.path.join(ROOT, "oracle")]
    env = dict(os.environ, GPUHASH_BATCH_BYTES=str(256 * 1024))
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [tuple(x) for x in out["got"]] == want
    runs = [tuple(x) for x in out["runs"]]
    assert len(runs) >= 3 and runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1
    assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))


# ---- 7. it is worth having ----

def test_batch_takes_at_most_half_the_loop(engine, tiny):
    """1,024 x [0, 9999]: one min_batch against a loop of 1,024 Engine.min calls over the same
    jobs, in this process; medians of five after a warm-up.  The loop is how this work is done
    without the batch call; the batch must take at most half its time.  (Measured on one MI355X:
    4.47 ms against 111.1 ms, ratio 0.040, kernel_ms 2.98)"""
    jobs, want = tiny

    def batch():
        t = time.perf_counter()
        got = engine.min_batch(jobs)
        return time.perf_counter() - t, got

    def loop():
        t = time.perf_counter()
        got = [engine.min(m, a, b) for m, a, b in jobs]
        return time.perf_counter() - t, got

    assert batch()[1] == want and loop()[1] == want  # warm-up, and both are right
    tb = statistics.median(batch()[0] for _ in range(5))
    kernel_ms = engine.stats()["kernel_ms"]
    tl = statistics.median(loop()[0] for _ in range(5))
    print(f"\nmin_batch {tb * 1e3:.2f} ms (kernel_ms {kernel_ms:.3f}), loop of {TINY} min calls {tl * 1e3:.2f} ms, "
          f"ratio {tb / tl:.3f}")
    assert tb <= 0.5 * tl, (tb, tl)
