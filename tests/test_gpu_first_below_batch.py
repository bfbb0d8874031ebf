"""GPU: gpuhash_first_below_batch -- many independent first-hit searches in one call, one scan
launch per digit count and kernel variant among them, in ascending digit order, each job
answered exactly as gpuhash_first_below answers it.

Expected values come from the oracle (tests/first_batch_jobs.py: oracle.hash_range + the first
index at or below the target) and from committed fixtures (tests/golden/min_batch.json,
tests/golden/first_below_batch.json); the engine is only ever compared WITH them, and with its
own Engine.first_below on the same job.
"""
import json
import os
import random
import statistics
import subprocess
import sys
import time

import pytest

import first_batch_jobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bitcoin-miner_amd", "lib", "gpuhash_cli")
U64 = (1 << 64) - 1
AUTO = 0


@pytest.fixture(scope="module")
def mix(oracle):
    return first_batch_jobs.jobs_and_answers(oracle)


def launch_keys(recs):
    return {(r["shard"], r["digits"], r["J"], r["C2"], r["EX"]) for r in recs}


def digits_never_decrease(recs):
    """Within one run (one context entry's records of one sub-batch, consecutive in the list)."""
    runs = {}
    for r in recs:
        runs.setdefault((r["shard"], r["lo"], r["hi"]), []).append(r["digits"])
    return all(d == sorted(d) for d in runs.values())


# ---- 1. parity ----

@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", first_batch_jobs.batch_jobs.POLICIES)
def test_parity_with_the_oracle_and_with_first_below(engine, mix, policy, rchunk):
    jobs, want = mix
    engine.set_layout_policy(policy)
    try:
        got = engine.first_below_batch(jobs, rchunk)
        st, recs = engine.stats(), engine.launches()
        single = [engine.first_below(m, a, b, t, rchunk) for m, a, b, t in jobs]
    finally:
        engine.set_layout_policy(AUTO)
    bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert got == single
    assert st["nonces"] == first_batch_jobs.examined(jobs, want)
    assert st["launches"] == len(recs) == len({(r["digits"], r["J"], r["C2"], r["EX"]) for r in recs})
    assert digits_never_decrease(recs), [r["digits"] for r in recs]
    assert all((r["lo"], r["hi"]) == (0, len(jobs) - 1) for r in recs)  # batch records: job indices


# ---- 2. edges ----

def test_edges(engine, oracle):
    import gpuhash
    top = oracle.hash(b"bradfitz", U64)
    assert engine.first_below_batch([(b"bradfitz", U64, U64, U64)]) == [(top, U64)]
    assert engine.stats()["nonces"] == 1
    assert engine.first_below_batch([(b"bradfitz", U64, U64, top), (b"bradfitz", U64, U64, top - 1)]) == [(top, U64), None]
    # a job that is not found leaves its outputs untouched: through the ABI, with marked arrays
    c = gpuhash.ctypes
    buf = c.create_string_buffer(b"msgmsg")
    off = (c.c_size_t * 3)(0, 3, 6)
    lo, hi, tg = (c.c_uint64 * 2)(0, 0), (c.c_uint64 * 2)(2, 2), (c.c_uint64 * 2)(0, U64)
    h, n, fd = (c.c_uint64 * 2)(7, 7), (c.c_uint64 * 2)(7, 7), (c.c_int * 2)(7, 7)
    rc = engine._lib.gpuhash_first_below_batch(engine._ctx, c.addressof(buf), off, 2, lo, hi, tg, h, n, fd)
    assert rc == 0 and list(fd) == [0, 1] and (h[0], n[0]) == (7, 7) and (h[1], n[1]) == (13781283048668101583, 0)
    assert engine.stats()["nonces"] == 3 + 1


def test_4096_single_nonce_jobs(engine, oracle):
    rng = random.Random("min-batch single nonces")  # test_gpu_min_batch.py's generator
    msgs = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 8, 42, 55, 61, 64, 120)))) for _ in range(64)]
    jobs, want = [], []
    for k in range(4096):
        n = rng.randrange(10 ** rng.randrange(0, 20)) if k % 7 else U64 - rng.randrange(3)
        h = oracle.hash(msgs[k % 64], n)
        jobs.append((msgs[k % 64], n, n, h - (k & 1)))  # the nonce's own hash, or that minus 1
        want.append(None if k & 1 else (h, n))
    assert engine.first_below_batch(jobs) == want
    st, recs = engine.stats(), engine.launches()
    assert st["nonces"] == 4096 and st["launches"] == len(recs) == len(launch_keys(recs))
    assert digits_never_decrease(recs)


def test_first_not_least(engine):
    # p1.pdf p.12: Hash("msg", 0..2) = 13781283048668101583, 4754799531757243342, 5611725180048225792
    jobs = [(b"msg", 0, 2, 13781283048668101583), (b"msg", 0, 2, 4754799531757243342),
            (b"msg", 0, 2, 4754799531757243341), (b"msg", 2, 2, U64)]
    assert engine.first_below_batch(jobs) == [(13781283048668101583, 0), (4754799531757243342, 1), None,
                                              (5611725180048225792, 2)]
    assert engine.stats()["nonces"] == 1 + 2 + 3 + 1


def test_a_span_over_the_maximum_is_refused_by_a_live_context_too(engine):
    import gpuhash
    with pytest.raises(ValueError):
        engine.first_below_batch([(b"x", 5, 5 + gpuhash.GPUHASH_BATCH_MAX_SPAN, 0)])


# ---- 3. a large job among small ones ----

def test_a_large_job_among_small_ones_keeps_its_own_bound_and_target(engine, oracle):
    with open(os.path.join(ROOT, "tests", "golden", "min_batch.json")) as f:
        g = {r["name"]: r for r in json.load(f)["ranges"]}["bradfitz_2p28"]
    big = (bytes.fromhex(g["msg_hex"]), g["lower"], g["upper"], g["hash"])
    assert big[:3] == (b"bradfitz", 0, (1 << 28) - 1) and oracle.hash(big[0], g["nonce"]) == g["hash"]
    rng = random.Random("first-below-batch large among small")
    small, want = [], []
    for k in range(100):
        lo = rng.randrange(10 ** rng.randrange(1, 12))
        m, cnt = b"other-%d" % k, rng.randrange(2, 3000)
        h = oracle.hash_range(m, lo, cnt)
        t = int(sorted(h.tolist())[cnt // 2])  # its own median hash
        small.append((m, lo, lo + cnt - 1, t))
        want.append(first_batch_jobs.first_index(h, lo, t))
    got = engine.first_below_batch(small[:50] + [big] + small[50:])
    # the golden nonce is the lowest nonce with the range's least hash: the first at or below it
    assert got[50] == (g["hash"], g["nonce"])
    # a shared bound would cut the small jobs short, a shared target find nothing in them
    assert got[:50] + got[51:] == want and all(w is not None for w in want)


# ---- 4. several context entries ----

def test_three_entries_give_the_same_results(mix):
    import gpuhash
    jobs, want = mix
    with gpuhash.Engine([0, 0, 0]) as eng:
        assert eng.first_below_batch(jobs) == want
        recs, st = eng.launches(), eng.stats()
        assert {r["shard"] for r in recs} == {0, 1, 2} and st["ndevices"] == 3
        runs = sorted({(r["lo"], r["hi"]) for r in recs})  # contiguous runs of whole jobs covering the batch
        assert runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1 and len(runs) == 3
        assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))
        assert st["launches"] == len(recs) == len(launch_keys(recs)) and digits_never_decrease(recs)
        assert st["nonces"] == first_batch_jobs.examined(jobs, want)


# ---- 5. sub-batches ----

CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import hash_oracle, first_batch_jobs, gpuhash
jobs, _ = first_batch_jobs.jobs_and_answers(hash_oracle.load_c_oracle())
with gpuhash.Engine([0]) as eng:
    got = eng.first_below_batch(jobs)
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
    assert [tuple(x) if x else None for x in out["got"]] == want
    runs = [tuple(x) for x in out["runs"]]
    assert len(runs) >= 3 and runs[0][0] == 0 and runs[-1][1] == len(jobs) - 1
    assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))


# ---- 6. the command-line client ----

def test_cli_batch_below(tmp_path):
    path = tmp_path / "jobs.txt"
    path.write_text("bradfitz 0 9999 1419516646206828\n\nbradfitz 0 9999 1419516646206827\n"
                    "msg 0 2 4754799531757243342\nmsg 2 2 0\n")
    out = subprocess.run([CLI, "--batch-below", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["Result 1419516646206828 9898", "None", "Result 4754799531757243342 1", "None"]
    path.write_text("bradfitz 0 9999\n")
    assert subprocess.run([CLI, "--batch-below", str(path)], capture_output=True).returncode == 2
    path.write_text("bradfitz 10 5 7\n")
    out = subprocess.run([CLI, "--batch-below", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "invalid argument" in out.stderr


# ---- 7. it is worth having ----

@pytest.fixture(scope="module")
def pow_jobs(oracle):
    """The 256 proof-of-work jobs of tests/golden/first_below_batch.json and its answers, 16 of
    them spot-checked against the oracle: the hash, and that none of the 1,000 nonces before the
    answer qualifies."""
    with open(os.path.join(ROOT, "tests", "golden", "first_below_batch.json")) as f:
        g = json.load(f)
    assert (g["lower"], g["upper"], g["target"], len(g["jobs"])) == (0, (1 << 32) - 1, (1 << 48) - 1, 256)
    jobs = [(b"pow-%04d" % k, 0, g["upper"], g["target"]) for k in range(256)]
    want = [(j["hash"], j["nonce"]) for j in g["jobs"]]
    assert [bytes.fromhex(j["msg_hex"]) for j in g["jobs"]] == [j[0] for j in jobs]
    for k in range(0, 256, 16):
        h, n = want[k]
        assert oracle.hash(jobs[k][0], n) == h <= g["target"]
        lo = max(0, n - 1000)
        if n > lo:
            assert int(oracle.hash_range(jobs[k][0], lo, n - lo).min()) > g["target"]
    return jobs, want


def test_batch_takes_at_most_half_the_loop(engine, pow_jobs):
    """256 stamps, (b"pow-%04d" % k, 0, 2^32-1, 2^48-1): one first_below_batch against a loop of 256
    Engine.first_below calls over the same jobs, in this process; medians of five after a warm-up.
    The loop is how this work is done without the batch call; the batch must take at most half
    its time.  (Measured on one MI355X: 9.32 ms against 101.5 ms, ratio 0.092, kernel_ms 7.62 in 40
    launches, four sub-batches of ten; another session 9.05 against 99.5 ms, 0.091.  DESIGN.md 3.12.)"""
    jobs, want = pow_jobs

    def batch():
        t = time.perf_counter()
        got = engine.first_below_batch(jobs)
        return time.perf_counter() - t, got

    def loop():
        t = time.perf_counter()
        got = [engine.first_below(m, a, b, tg) for m, a, b, tg in jobs]
        return time.perf_counter() - t, got

    assert batch()[1] == want and loop()[1] == want  # warm-up, and both are right
    tb = statistics.median(batch()[0] for _ in range(5))
    st, recs = engine.stats(), engine.launches()
    tl = statistics.median(loop()[0] for _ in range(5))
    print(f"\nfirst_below_batch {tb * 1e3:.2f} ms (kernel_ms {st['kernel_ms']:.3f}, {st['launches']} launches, "
          f"sum of their ms {sum(r['ms'] for r in recs):.3f}, wall_ms {st['wall_ms']:.3f}), "
          f"loop of 256 first_below calls {tl * 1e3:.2f} ms, ratio {tb / tl:.3f}")
    assert tb <= 0.5 * tl, (tb, tl)
