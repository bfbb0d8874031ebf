"""GPU: the packed kernel for tiny batch jobs -- gpuhash_min_batch and gpuhash_collect_below_batch
under GPUHASH_LAYOUT_PACKED_ALWAYS: every lane hashes one (job, nonce).

Expected values come from the oracle (tests/packed_jobs.py, tests/batch_jobs.py,
tests/collect_batch_jobs.py); the engine is only ever compared WITH them, and with its own
unflagged call on the same jobs.
"""
import json
import os
import random
import statistics
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import batch_jobs
import collect_batch_jobs
import packed_jobs
from packed_jobs import MAX_SPAN, PACKED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "bitcoin-miner_amd"), os.path.join(ROOT, "oracle")]
U64 = (1 << 64) - 1
AUTO = 0
TINY = 1024  # jobs [0, 9999], one 8-byte message each
ECANCELED = -6


@pytest.fixture(scope="module")
def one():
    """One context entry on device 0, so that `one launch` means the same on any machine; the
    policy is AUTO again after every test."""
    import gpuhash
    e = gpuhash.Engine([0])
    yield e
    e.close()


@pytest.fixture()
def packed(one):
    one.set_layout_policy(PACKED)
    yield one
    one.set_layout_policy(AUTO)


@pytest.fixture(scope="module")
def mix(oracle):
    named = batch_jobs.job_mix()
    return [(m, a, b) for _, m, a, b in named], batch_jobs.expected(oracle, named)


@pytest.fixture(scope="module")
def cmix(oracle):
    return collect_batch_jobs.jobs_and_answers(oracle)


@pytest.fixture(scope="module")
def tiny(oracle):
    jobs = [(b"job-%04d" % k, 0, 9999) for k in range(TINY)]
    return jobs, [oracle.min(m, a, b) for m, a, b in jobs]


def variants(eng):
    return [(r["J"], r["C2"], r["EX"]) for r in eng.launches()]


# ---- 1. the class matrix ----

def test_class_matrix_in_one_launch_each(packed, oracle):
    jobs = packed_jobs.matrix()
    hs = packed_jobs.hashes(oracle, jobs)
    got = packed.min_batch(jobs)
    want = packed_jobs.expected_min(hs, jobs)
    bad = [(k, len(jobs[k][0]), jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    recs = packed.launches()
    assert len(recs) == 1 and variants(packed) == [(-1, 4, 0)], recs
    assert (recs[0]["digits"], recs[0]["c"], recs[0]["lo"], recs[0]["hi"]) == (0, 2, 0, len(jobs) - 1)
    assert recs[0]["nonces"] == packed.stats()["nonces"] == sum(b - a + 1 for _, a, b in jobs)
    targets = packed_jobs.quartile_targets(hs)
    got = packed.collect_below_batch([(m, a, b, t, 5) for (m, a, b), t in zip(jobs, targets)])
    want = packed_jobs.expected_collect(hs, jobs, targets)
    bad = [(k, len(jobs[k][0]), jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert variants(packed) == [(-1, 4, 0)]


# ---- 2. the shared mixes ----

@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_min_mix_under_the_flag(one, mix, policy):
    jobs, want = mix
    try:
        one.set_layout_policy(policy)
        plain, nonces = one.min_batch(jobs), one.stats()["nonces"]
        one.set_layout_policy(policy | PACKED)
        got = one.min_batch(jobs)
        st = one.stats()
    finally:
        one.set_layout_policy(AUTO)
    bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert got == plain and st["nonces"] == nonces == sum(b - a + 1 for _, a, b in jobs)
    assert variants(one) == [(-1, 4, 0)] and st["launches"] == 1


def test_collect_mix_under_the_flag(one, cmix):
    jobs, want = cmix
    plain, nonces = one.collect_below_batch(jobs), one.stats()["nonces"]
    try:
        one.set_layout_policy(PACKED)
        got = one.collect_below_batch(jobs)
        st = one.stats()
        counts = one.count_below_batch([j[:4] for j in jobs])
    finally:
        one.set_layout_policy(AUTO)
    bad = [(k, jobs[k][1:], g[0], w[0]) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert got == plain and st["nonces"] == nonces
    assert counts == [w[0] for w in want]


# ---- 3. many tiny jobs ----

def test_1024_config1_sized_jobs_are_one_launch(packed, tiny):
    jobs, want = tiny
    assert packed.min_batch(jobs) == want
    st, recs = packed.stats(), packed.launches()
    assert st["launches"] == len(recs) == 1 and variants(packed) == [(-1, 4, 0)]
    assert recs[0]["nonces"] == 10000 * TINY == st["nonces"]
    assert (recs[0]["lo"], recs[0]["hi"]) == (0, TINY - 1)
    assert (recs[0]["digits"], recs[0]["c"]) == (0, 1)


# ---- 4. single nonces ----

def test_4096_single_nonce_jobs(packed, oracle):
    rng = random.Random("min-batch single nonces")
    msgs = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 8, 42, 55, 61, 64, 120)))) for _ in range(64)]
    jobs = []
    for k in range(4096):
        n = rng.randrange(10 ** rng.randrange(0, 20)) if k % 7 else U64 - rng.randrange(3)
        jobs.append((msgs[k % 64], n, n))
    assert any(n == U64 for _, n, _ in jobs)
    assert packed.min_batch(jobs) == [(oracle.hash(m, n), n) for m, n, _ in jobs]
    st = packed.stats()
    assert st["launches"] == 1 and st["nonces"] == 4096 and variants(packed) == [(-1, 4, 0)]


# ---- 5. the cap ----

def test_the_cap_splits_one_batch_between_both_kinds(packed, oracle):
    rng = random.Random("packed cap")
    small = []
    for k in range(50):
        lo = rng.randrange(10 ** rng.randrange(1, 12))
        small.append((b"other-%d" % k, lo, lo + rng.randrange(1, 3000)))
    at = (b"bradfitz", 10 ** 9 - (1 << 19), 10 ** 9 + (1 << 19) - 1)   # 2^20 nonces across a digit boundary
    over = (b"bradfitz", 10 ** 9 - (1 << 19), 10 ** 9 + (1 << 19))     # 2^20 + 1
    assert at[2] - at[1] + 1 == MAX_SPAN
    jobs = small[:25] + [at, over] + small[25:]
    got = packed.min_batch(jobs)
    h = oracle.hash_range(b"bradfitz", over[1], MAX_SPAN + 1)
    i, j = int(np.argmin(h[:-1])), int(np.argmin(h))
    assert got[25] == (int(h[i]), at[1] + i) and got[26] == (int(h[j]), over[1] + j)
    assert got[:25] + got[27:] == [oracle.min(m, a, b) for m, a, b in small]
    recs = packed.launches()
    kinds = [r["C2"] for r in recs]
    assert kinds.count(4) == 1 and kinds[-1] == 4 and len(kinds) > 1, recs
    assert recs[-1]["nonces"] == MAX_SPAN + sum(b - a + 1 for _, a, b in small)
    assert sum(r["nonces"] for r in recs[:-1]) == MAX_SPAN + 1


# ---- 6. ties ----

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
    with gpuhash.Engine([0], lib_path=gpuhash.TIETEST_LIB_PATH) as eng:
        assert b"TIE-TEST" in eng._lib.gpuhash_version()
        eng.set_layout_policy(PACKED)
        assert eng.min_batch([jobs[i] for i in order]) == [want[i] for i in order]
        assert variants(eng) == [(-1, 4, 0)]


# ---- 7. several context entries ----

def test_three_entries_give_the_same_results(mix, tiny, cmix):
    import gpuhash
    with gpuhash.Engine([0, 0, 0]) as eng:
        eng.set_layout_policy(PACKED)
        for jobs, want in (mix, tiny):
            assert eng.min_batch(jobs) == want
            recs, st = eng.launches(), eng.stats()
            assert {r["shard"] for r in recs} == {0, 1, 2} and st["ndevices"] == 3
            assert all(r["C2"] == 4 for r in recs) and st["launches"] == len(recs) == 3
            runs = sorted({(r["lo"], r["hi"]) for r in recs})
            assert runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1
            assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))
        jobs, want = cmix
        assert eng.collect_below_batch(jobs) == want


# ---- 8, 9. sub-batches; a short collect list ----

CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import batch_jobs, collect_batch_jobs, gpuhash, hash_oracle
oracle = hash_oracle.load_c_oracle()
jobs = [(m, a, b) for _, m, a, b in batch_jobs.job_mix()]
tiny = [(b"job-%04d" % k, 0, 9999) for k in range(1024)]
cjobs, _ = collect_batch_jobs.jobs_and_answers(oracle)
with gpuhash.Engine([0]) as eng:
    eng.set_layout_policy(64)
    out = {{"mix": eng.min_batch(jobs)}}
    out["tiny"] = eng.min_batch(tiny)
    out["runs"] = sorted({{(r["lo"], r["hi"]) for r in eng.launches()}})
    out["kinds"] = sorted({{r["C2"] for r in eng.launches()}})
    out["collect"] = eng.collect_below_batch(cjobs)
    out["collect_kinds"] = [r["C2"] for r in eng.launches()]
    print(json.dumps(out))
"""


def child(env):
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=PATHS)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_sub_batches_on_the_device(mix, tiny):
    """GPUHASH_BATCH_BYTES = 256 KiB in a fresh child process: the 1,024 tiny jobs, about 5 KiB of
    tables and list entries each, are cut into many sub-batches, every one a packed launch."""
    out = child({"GPUHASH_BATCH_BYTES": str(256 * 1024)})
    assert [tuple(x) for x in out["mix"]] == mix[1] and [tuple(x) for x in out["tiny"]] == tiny[1]
    runs = [tuple(x) for x in out["runs"]]
    assert len(runs) >= 3 and runs[0][0] == 0 and runs[-1][1] == TINY - 1 and out["kinds"] == [4]
    assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))


def test_a_short_list_cuts_jobs_short_and_they_are_re_run(cmix):
    """GPUHASH_COLLECT_BUFFER = 64 in a fresh child: the packed launch lists 64 hits of thousands,
    and every job it cut short is re-run alone, through the unpacked single path."""
    jobs, want = cmix
    out = child({"GPUHASH_COLLECT_BUFFER": "64"})
    got = [(t, [tuple(h) for h in hits]) for t, hits in out["collect"]]
    assert got == want
    kinds = out["collect_kinds"]
    assert kinds[0] == 4 and len(kinds) > 1 and 4 not in kinds[1:], kinds[:8]


# ---- 10. cancel ----

def test_cancel_inside_the_packed_launch(one, mix):
    """4,096 jobs of 2^20 nonces, 4.3 G nonces in some sixty sub-batches: left alone 0.23 s of
    kernel time at the packed kernel's measured 18.5 GH/s, and their staging.
    Cancelled the first time progress() shows work handed out; the call is made once, and the mix
    right after it is exact.  Measured on one MI355X: cancelled at 2,621,440 of 4,294,967,296
    nonces, the call returned after 6.6 ms."""
    import gpuhash
    jobs = [(b"cancel-%04d" % k, 10 ** 7, 10 ** 7 + MAX_SPAN - 1) for k in range(4096)]
    n, data, off, lower, upper, _ = one._batch_arrays(jobs, 0, 3)
    sent = 0x5A5A5A5A5A5A5A5A
    hashes, nonces = (gpuhash.ctypes.c_uint64 * n)(*[sent] * n), (gpuhash.ctypes.c_uint64 * n)(*[sent] * n)
    out = {}

    def call():
        t = time.perf_counter()
        out["rc"] = one._lib.gpuhash_min_batch(one._ctx, gpuhash.ctypes.addressof(data), off, n, lower, upper,
                                               hashes, nonces)
        out["wall"] = time.perf_counter() - t

    one.set_layout_policy(PACKED)
    try:
        th = threading.Thread(target=call)
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
        print(f"\ncancelled at {cancelled}, the call took {out['wall'] * 1e3:.1f} ms")
        assert cancelled is not None and cancelled[1] == 4096 * MAX_SPAN
        assert out["rc"] == ECANCELED
        assert all(v == sent for v in hashes) and all(v == sent for v in nonces)
        assert one.min_batch(mix[0]) == mix[1]
        assert variants(one) == [(-1, 4, 0)]
    finally:
        one.resume()
        one.set_layout_policy(AUTO)


# ---- 11. it is worth having ----

def test_packed_tiny_batch_is_faster_beyond_the_noise(one, tiny):
    """1,024 x [0, 9999] through min_batch, flagged against unflagged, alternating on one engine in
    one process; medians of five wall times after a warm-up each.  The unflagged call is the code
    path of the commit before the flag, byte for byte.  The flagged median must lie below the
    unflagged one by more than three times the unflagged runs' own spread (max - min of the five).
    Measured on one MI355X: packed 1.73 ms (kernel_ms 0.728), unflagged 4.46 ms
    (kernel_ms 3.051, spread 0.25 ms), ratio 0.389."""
    jobs, want = tiny

    def run(policy):
        one.set_layout_policy(policy)
        t = time.perf_counter()
        got = one.min_batch(jobs)
        return time.perf_counter() - t, got, one.stats()["kernel_ms"]

    try:
        assert run(PACKED)[1] == want and run(AUTO)[1] == want  # warm-up, and both are right
        tf, tu, kf, ku = [], [], [], []
        for _ in range(5):
            t, _, k = run(PACKED)
            tf.append(t)
            kf.append(k)
            t, _, k = run(AUTO)
            tu.append(t)
            ku.append(k)
    finally:
        one.set_layout_policy(AUTO)
    mf, mu, spread = statistics.median(tf), statistics.median(tu), max(tu) - min(tu)
    print(f"\nmin_batch of {TINY} x [0, 9999]: packed {mf * 1e3:.2f} ms (kernel_ms {statistics.median(kf):.3f}), "
          f"unflagged {mu * 1e3:.2f} ms (kernel_ms {statistics.median(ku):.3f}, spread {spread * 1e3:.2f} ms), "
          f"ratio {mf / mu:.3f}")
    assert mf < mu - 3 * spread, (mf, mu, spread)
