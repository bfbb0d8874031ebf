"""GPU: gpuhash_collect_below -- every nonce of a range whose hash is at or below a target,
counted exactly, and the lowest `cap` of them listed -- through the C ABI, against the oracle.

Expected values are numpy over oracle.hash_range(...), never the engine's own output: the
total is the number of hashes <= target, and the list is exactly the lowest min(cap, total)
qualifying nonces, ascending, under every layout policy, work-item granularity, shard and
slice split, and when the device list overflows.
"""
import os
import random
import statistics
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
COLLECT_MAX = 1 << 20
M120 = (b"The quick brown fox jumps over the lazy dog. " * 3)[:120]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bitcoin-miner_amd", "lib", "gpuhash_cli")


def expected(h, lo, target, cap=COLLECT_MAX):
    """(total, [(hash, nonce), ...] of the lowest min(cap, total) hits, ascending by nonce)."""
    idx = np.nonzero(h <= np.uint64(target))[0]
    return int(idx.size), [(int(h[i]), lo + int(i)) for i in idx[:cap]]


def five_targets(h):
    """The window's minimum hash minus 1 (nothing qualifies), the minimum (one hit), about the
    1/1000 and the 1/64 quantiles, and 2^64-1 (every nonce)."""
    s = np.sort(h)
    return [int(s[0]) - 1, int(s[0]), int(s[max(len(s) // 1000, 1)]), int(s[len(s) // 64]), U64]


def test_spec_example(engine):
    # p1.pdf p.12: Hash("msg", 0..2) = 13781283048668101583, 4754799531757243342, 5611725180048225792
    assert engine.collect_below(b"msg", 0, 2, 5611725180048225792) == \
        (2, [(4754799531757243342, 1), (5611725180048225792, 2)])
    assert engine.stats()["nonces"] == 3
    assert engine.collect_below(b"msg", 0, 2, U64, cap=1) == (3, [(13781283048668101583, 0)])
    assert engine.collect_below(b"msg", 0, 2, 4754799531757243341) == (0, [])
    assert engine.count_below(b"msg", 0, 2, 4754799531757243342) == 1  # cap = 0, null arrays


def test_errors_are_loud(engine):
    import gpuhash
    with pytest.raises(gpuhash.GpuHashError) as e:
        engine.collect_below(b"x", 5, 4, 7)
    assert e.value.rc == gpuhash.GPUHASH_EINVAL
    with pytest.raises(ValueError):
        engine.collect_below(b"x", 0, 4, 1 << 64)
    with pytest.raises(ValueError):
        engine.collect_below(b"x", 0, 4, 7, cap=COLLECT_MAX + 1)


def variant_cases():
    """variant_cases() of test_gpu_first_below.py, restated: (msg, lower, count) windows with a
    seeded random digit count per message length 0..140, most of them across a digit-count
    boundary, and fixed windows at 0, at 10^19 and at the top of uint64.  test_every_variant
    checks the layout families these reach, not every J: the guarantee that every compiled
    (J, C2, EX, MODE) kernel runs is tests/test_gpu_variant_matrix.py's."""
    rng = random.Random(42)
    cases = []
    for mlen in list(range(0, 70)) + list(range(100, 141, 3)):
        m = bytes(rng.randrange(256) for _ in range(mlen))
        d = rng.choice([3, 5, 7, 9, 10, 11, 12, 13])
        cases.append((m, max(0, 10 ** d - rng.randrange(1, 3000)), rng.randrange(1000, 6000)))
    for m in (b"", b"bradfitz", M120, M120[:44], M120[:45]):
        cases.append((m, 0, 12000))
        cases.append((m, U64 - 4999, 5000))
        cases.append((m, 10 ** 19 - 2500, 5000))
    return cases


def test_every_variant(engine, oracle):
    seen = set()
    for m, lo, cnt in variant_cases():
        h = oracle.hash_range(m, lo, cnt)
        for ti, target in enumerate(five_targets(h)):
            for cap in (COLLECT_MAX, 7):
                want = expected(h, lo, target, cap)
                assert ti not in (0, 1, 4) or want[0] == {0: 0, 1: 1, 4: cnt}[ti]
                got = engine.collect_below(m, lo, lo + cnt - 1, target, cap=cap)
                assert got == want, (len(m), lo, cnt, ti, target, cap)
                assert engine.stats()["nonces"] == cnt
        seen |= {(min(r["J"], 2), r["C2"], r["EX"]) for r in engine.launches()}
    # plain (J = 0, 1, >= 2), K+W table, classic straddle, extra block; AUTO takes the lane
    # table / two-word loop only for wider searches (test_forced_layouts drives those)
    assert {(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 0), (2, 0, 1)} <= seen, seen


def _forced_cases():
    import gpuhash as g
    cases = []
    # the (mlen, digits) pairs of test_gpu.py's forced-layout tests and the variant each forces
    for mlen, d, c2, j in [(58, 10, 2, 1), (59, 10, 2, 1), (60, 10, 2, 1), (56, 12, 2, 1), (59, 12, 2, 1),
                           (120, 10, 1, 0), (54, 10, 1, 0), (119, 12, 1, 0)]:
        cases.append(("uniform", g.LAYOUT_UNIFORM, mlen, d, (c2, j)))
    for mlen, d in [(61, 10), (61, 7), (62, 8), (62, 6), (125, 9), (126, 9)]:
        cases.append(("lanetable", g.LAYOUT_LANETABLE, mlen, d, (3, 1)))
    for mlen, d in [(59, 12), (58, 10)]:
        cases.append(("classic", g.LAYOUT_CLASSIC, mlen, d, (1, 1)))
    for mlen, d, j in [(8, 12, 4), (8, 8, 3), (12, 12, 5), (27, 9, 8), (42, 14, 13), (46, 14, 14), (42, 18, 14)]:
        cases.append(("tail", g.LAYOUT_AUTO | g.LAYOUT_TAIL_ALWAYS, mlen, d, (0, j)))
    return cases


@pytest.mark.parametrize("case", _forced_cases(), ids=lambda c: f"{c[0]}-{c[2]}-{c[3]}")
def test_forced_layouts(engine, oracle, case, request):
    import gpuhash
    name, policy, mlen, d, (c2, j) = case
    rng = random.Random(f"{name} {mlen} {d}")
    m = bytes(rng.randrange(32, 127) for _ in range(mlen))
    size = 60_000 if d <= 6 else rng.choice([60_000, 120_000, 250_000, 400_000])
    # inside digit group d, across a multiple of 10^5 (10^4 for d = 6): loop-word roll-overs,
    # several rows, and for the lane table several loop values
    B = 10 ** min(5, d - 2)
    base = 10 ** (d - 1) + 5 * 10 ** (d - 2) + rng.randrange(10 ** (d - 2))
    lo = base - base % B - size // 3
    hi = lo + size - 1
    assert 10 ** (d - 1) <= lo and hi < 10 ** d
    h = oracle.hash_range(m, lo, size)
    s = np.sort(h)
    request.addfinalizer(lambda: engine.set_layout_policy(gpuhash.LAYOUT_AUTO))
    engine.set_layout_policy(policy)
    for target in (int(s[2]), int(s[size // 64])):  # total 3, and the 1/64 quantile
        want = expected(h, lo, target)
        assert want[0] == (3 if target == int(s[2]) else size // 64 + 1)
        for rchunk in (0, 10):
            assert engine.collect_below(m, lo, hi, target, rchunk=rchunk) == want, (name, mlen, d, rchunk)
            recs = engine.launches()
            if name == "tail":
                assert {(r["J"], r["digits"]) for r in recs} == {(j, d)}, recs
            else:
                assert any((r["C2"], r["J"]) == (c2, j) for r in recs), recs
            assert engine.stats()["nonces"] == size


@pytest.mark.parametrize("m", [b"", b"bradfitz", M120[:50]], ids=["empty", "bradfitz", "two-blocks"])
def test_top_of_u64(engine, oracle, m):
    """A nonce of 2^64-1 is a legal hit, and the last nonce of the range is not lost."""
    lo = U64 - 4999
    h = oracle.hash_range(m, lo, 5000)
    for target in five_targets(h) + [int(h[-1])]:
        want = expected(h, lo, target)
        assert engine.collect_below(m, lo, U64, target) == want
        assert engine.stats()["nonces"] == 5000
        assert engine.count_below(m, lo, U64, target) == want[0]
    assert expected(h, lo, U64)[1][-1] == (int(h[-1]), U64)
    assert engine.collect_below(m, U64, U64, U64) == (1, [(int(h[-1]), U64)])
    assert engine.collect_below(m, U64, U64, int(h[-1])) == (1, [(int(h[-1]), U64)])
    assert engine.collect_below(m, U64, U64, int(h[-1]) - 1) == (0, [])
    assert engine.stats()["nonces"] == 1


def test_device_list_overflow(oracle, monkeypatch):
    """GPUHASH_COLLECT_BUFFER=64: a range with more hits than the device list holds is split
    and run again, and the answer is still exact."""
    import gpuhash
    monkeypatch.setenv("GPUHASH_COLLECT_BUFFER", "64")
    m, lo, size = b"bradfitz", 123_450_000, 20_000
    hi = lo + size - 1
    h = oracle.hash_range(m, lo, size)
    with gpuhash.Engine([0]) as one:
        # every nonce a hit, the first 1000 wanted
        assert one.collect_below(m, lo, hi, U64, cap=1000) == expected(h, lo, U64, 1000)
        ranges = {(r["lo"], r["hi"]) for r in one.launches()}
        assert (lo, hi) in ranges and (lo, lo + (size - 1) // 2) in ranges and len(ranges) > 16, sorted(ranges)
        assert all(lo <= a <= b <= hi for a, b in ranges)
        assert one.stats()["nonces"] == size
        # once the output is full nothing is re-run: a pure count is one run of the range
        assert one.count_below(m, lo, hi, U64) == size
        assert {(r["lo"], r["hi"]) for r in one.launches()} == {(lo, hi)}
        # about 313 hits against a list of 64, all wanted
        target = int(np.sort(h)[size // 64])
        want = expected(h, lo, target)
        assert want[0] == size // 64 + 1
        assert one.collect_below(m, lo, hi, target) == want
        assert len({(r["lo"], r["hi"]) for r in one.launches()}) > 4
        assert one.collect_below(m, lo, hi, target, cap=5, rchunk=7) == expected(h, lo, target, 5)


def test_shards(oracle):
    """Two contiguous shards (a context opened on [0, 0]): hits only in the upper shard, hits
    in both, and cap filled inside the lower shard."""
    import gpuhash
    m, size = b"bradfitz", 200_000
    with gpuhash.Engine([0, 0]) as two:
        done = set()
        for k in range(1, 40):
            lo = k * 1_000_000
            hi = lo + size - 1
            (a0, a1), (b0, b1) = gpuhash.shard_range(len(m), lo, hi, 2)
            assert a0 == lo and b0 == a1 + 1 and b1 == hi
            h = oracle.hash_range(m, lo, size)
            low_min, up_min = int(h[:b0 - lo].min()), int(h[b0 - lo:].min())
            if up_min < low_min and "upper" not in done:
                done.add("upper")
                want = expected(h, lo, up_min)
                assert want[0] == 1 and want[1][0][1] >= b0
                assert two.collect_below(m, lo, hi, up_min) == want
                assert {r["shard"] for r in two.launches()} == {0, 1}
            if "both" not in done:
                done.add("both")
                target = int(np.sort(h)[size // 1000])
                want = expected(h, lo, target)
                nlow = int((h[:b0 - lo] <= np.uint64(target)).sum())
                assert 0 < nlow < want[0] == size // 1000 + 1
                assert two.collect_below(m, lo, hi, target) == want
                assert {r["shard"] for r in two.launches()} == {0, 1}
                assert two.stats()["ndevices"] == 2
                # cap filled inside the lower shard: the upper shard's hits are only counted
                assert two.collect_below(m, lo, hi, target, cap=nlow - 1) == expected(h, lo, target, nlow - 1)
                assert {r["shard"] for r in two.launches()} == {0, 1}
                assert two.count_below(m, lo, hi, target) == want[0]
            if done == {"upper", "both"}:
                break
        assert done == {"upper", "both"}


def test_slices(oracle, monkeypatch):
    """GPUHASH_SLICE_NONCES=50000 over 250,000 nonces: the total is the sum over five slices
    and the list is ascending across slice borders."""
    import gpuhash
    monkeypatch.setenv("GPUHASH_SLICE_NONCES", "50000")
    m, lo, size = b"bradfitz", 7_250_000, 250_000
    h = oracle.hash_range(m, lo, size)
    target = int(np.sort(h)[size // 1000])
    want = expected(h, lo, target)
    per_slice = [int((h[i:i + 50_000] <= np.uint64(target)).sum()) for i in range(0, size, 50_000)]
    assert sum(per_slice) == want[0] == 251 and sum(1 for c in per_slice if c) >= 4
    with gpuhash.Engine([0]) as one:
        assert one.collect_below(m, lo, lo + size - 1, target) == want
        assert {r["lo"] for r in one.launches()} == {lo + i for i in range(0, size, 50_000)}
        assert one.stats()["nonces"] == size
        # cap reached in the first slice that has hits: the later slices are still counted
        assert one.collect_below(m, lo, lo + size - 1, target, cap=1) == expected(h, lo, target, 1)
        assert {r["lo"] for r in one.launches()} == {lo + i for i in range(0, size, 50_000)}


@pytest.fixture(scope="module")
def tie_engine():
    import gpuhash
    if not os.path.exists(gpuhash.TIETEST_LIB_PATH):
        pytest.fail("libgpuhash_tietest.so not built (make -C bitcoin-miner_amd)")
    eng = gpuhash.Engine(lib_path=gpuhash.TIETEST_LIB_PATH)
    yield eng
    eng.close()


def truncated(oracle, msg, lo, count):
    """The hashes as the tie-test build keeps them (test_gpu_ties.py): the top 4 bits."""
    h = oracle.hash_range(msg, lo, count)
    return (h >> np.uint64(60)) << np.uint64(32)


def test_dense_hits_on_the_tie_test_build(tie_engine, oracle):
    """libgpuhash_tietest.so keeps 4 bits of each hash, so at the truncated target 3 << 32 a
    quarter of all nonces are hits: hits in every wave iteration, full and nearly full
    ballots, which real 64-bit hashes never reach at a sparse target."""
    assert b"TIE-TEST" in tie_engine._lib.gpuhash_version()
    target = 3 << 32
    for m, lo, n in [(b"bradfitz", 999_990_000, 20_000), (M120, 9_999_990_000, 20_000), (b"x" * 53, 0, 20_000),
                     (b"y" * 61, 999_900_000, 300_000)]:
        k = truncated(oracle, m, lo, n)
        want = expected(k, lo, target)
        assert 0.2 * n < want[0] < 0.3 * n
        assert tie_engine.collect_below(m, lo, lo + n - 1, target) == want, (m, lo, n)
        assert tie_engine.collect_below(m, lo, lo + n - 1, target, cap=100, rchunk=7) == expected(k, lo, target, 100)
        assert tie_engine.count_below(m, lo, lo + n - 1, target) == want[0]
        # every nonce: all 64 lanes of every ballot
        assert tie_engine.collect_below(m, lo, lo + n - 1, 15 << 32) == expected(k, lo, 15 << 32)


def test_count_below_is_the_total(engine, oracle):
    m, lo, n = M120, 999_990_000, 30_000
    h = oracle.hash_range(m, lo, n)
    for target in five_targets(h):
        total, hits = engine.collect_below(m, lo, lo + n - 1, target)
        assert engine.count_below(m, lo, lo + n - 1, target) == total == expected(h, lo, target)[0]
        assert engine.stats()["nonces"] == n


def test_cli_all_below(oracle):
    h = oracle.hash_range(b"bradfitz", 0, 10000)
    for target, cap in ((1 << 52, None), (1419516646206828, None), (1419516646206827, None), (U64, 3)):
        total, hits = expected(h, 0, target, cap or COLLECT_MAX)
        out = subprocess.run([CLI, "--all-below", "bradfitz", "0", "9999", str(target)] + ([str(cap)] if cap else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.splitlines() == [f"Total {total}"] + [f"Hit {hh} {nn}" for hh, nn in hits]
    assert expected(h, 0, 1 << 52)[0] == 2
    out = subprocess.run([CLI, "--all-below", "bradfitz", "10", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "invalid argument" in out.stderr
    out = subprocess.run([CLI, "--all-below", "bradfitz", "0", "9", "7", str(COLLECT_MAX + 1)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "invalid argument" in out.stderr
    assert subprocess.run([CLI, "--all-below", "bradfitz", "0", "9999"], capture_output=True).returncode == 2
    assert subprocess.run([CLI, "--all-below", "bradfitz", "0", "9999", "x"], capture_output=True).returncode == 2


def test_sparse_collect_costs_a_min_search(engine):
    """bradfitz over [0, 2^32-1] at target 2^40 (about 256 expected hits): the collecting scan
    costs what gpuhash_min costs on the same range, whose code this feature does not touch.
    Medians of five kernel_ms each, after a warm-up.  The bound is the larger of 2% and three
    times gpuhash_min's own spread ((max - min) / median of its five runs) in this test: a
    spill or a lost wave of occupancy in the collecting kernels costs far more than that.
    Measured (build 652fbb565b95d16a): collect_below 124.038 ms (spread 0.13%),
    gpuhash_min 123.874 ms (spread 0.05%), ratio 1.0013; the session before 124.498 against
    124.322 ms, ratio 1.0014.  The bound was 2% both times."""
    import gpuhash
    m, hi, target = b"bradfitz", (1 << 32) - 1, 1 << 40
    total, hits = engine.collect_below(m, 0, hi, target)  # warm-up: code objects, buffers
    engine.min(m, 0, hi)
    t_collect, t_min = [], []
    for _ in range(5):
        assert engine.collect_below(m, 0, hi, target) == (total, hits)
        t_collect.append(engine.stats()["kernel_ms"])
        engine.min(m, 0, hi)
        t_min.append(engine.stats()["kernel_ms"])
    med_c, med_m = statistics.median(t_collect), statistics.median(t_min)
    spread_m = (max(t_min) - min(t_min)) / med_m
    spread_c = (max(t_collect) - min(t_collect)) / med_c
    bound = max(0.02, 3 * spread_m)
    print(f"collect_below median {med_c:.3f} ms (spread {spread_c * 100:.2f}%), gpuhash_min median {med_m:.3f} ms "
          f"(spread {spread_m * 100:.2f}%), ratio {med_c / med_m:.4f}, bound {1 + bound:.4f}, hits {total}, "
          f"build {gpuhash.build_id()}")
    # oracle-free invariants of the list
    assert total == len(hits) and 128 <= total <= 512  # 256 expected, +-8 sigma
    assert [n for _, n in hits] == sorted({n for _, n in hits})
    for hh, nn in hits:
        assert hh <= target and 0 <= nn <= hi and gpuhash.Hash(m, nn) == hh
    assert engine.stats()["nonces"] == 1 << 32
    assert engine.count_below(m, 0, hi, 0) == 0
    assert med_c <= med_m * (1 + bound), (med_c, med_m, bound)
