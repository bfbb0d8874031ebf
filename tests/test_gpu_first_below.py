"""GPU: gpuhash_first_below -- the lowest nonce of a range whose hash is at or below a target
-- through the C ABI, against the oracle.

Expected values are the first index of oracle.hash_range(...) with hash <= target (numpy),
or the committed golden; never the engine's own output.  Every answer must be the LOWEST
qualifying nonce, under every layout policy, work-item granularity, shard and slice split.
"""
import os
import random
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
M120 = (b"The quick brown fox jumps over the lazy dog. " * 3)[:120]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bitcoin-miner_amd", "lib", "gpuhash_cli")


def first_index(h, lo, target):
    """What an ascending scan that stops at its first hit returns."""
    idx = np.nonzero(h <= np.uint64(target))[0]
    return None if idx.size == 0 else (int(h[idx[0]]), lo + int(idx[0]))


def five_targets(h):
    """The window's minimum hash, that minus 1 (nothing qualifies), about the 1/64 and the
    1/1000 quantiles, and 2^64-1."""
    s = np.sort(h)
    return [int(s[0]), int(s[0]) - 1, int(s[len(s) // 64]), int(s[max(len(s) // 1000, 1)]), U64]


def test_first_not_least(engine):
    # p1.pdf p.12: Hash("msg", 0..2) = 13781283048668101583, 4754799531757243342, 5611725180048225792:
    # nonce 0 already meets the target, while the minimum of the range (gpuhash_min's answer) is at 1
    assert engine.first_below(b"msg", 0, 2, 13781283048668101583) == (13781283048668101583, 0)
    assert engine.stats()["nonces"] == 1
    assert engine.min(b"msg", 0, 2) == (4754799531757243342, 1)
    assert engine.first_below(b"msg", 0, 2, 4754799531757243342) == (4754799531757243342, 1)
    assert engine.first_below(b"msg", 0, 2, 4754799531757243341) is None
    assert engine.stats()["nonces"] == 3
    assert engine.first_below(b"msg", 2, 2, U64) == (5611725180048225792, 2)


def test_errors_are_loud(engine):
    import gpuhash
    with pytest.raises(gpuhash.GpuHashError) as e:
        engine.first_below(b"x", 5, 4, 7)
    assert e.value.rc == gpuhash.GPUHASH_EINVAL
    with pytest.raises(ValueError):
        engine.first_below(b"x", 0, 4, 1 << 64)


def variant_cases():
    """The window family of test_gpu.py's test_hash_range_bit_exact, restated: (msg, lower,
    count) windows with a seeded random digit count per message length 0..140, most of them
    across a digit-count boundary, and fixed windows at 0, at 10^19 and at the top of uint64.
    test_every_variant checks the layout families these reach, not every J: the guarantee that
    every compiled (J, C2, EX, MODE) kernel runs is tests/test_gpu_variant_matrix.py's."""
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
            want = first_index(h, lo, target)
            got = engine.first_below(m, lo, lo + cnt - 1, target)
            assert got == want, (len(m), lo, cnt, ti, target)
            assert engine.stats()["nonces"] == (cnt if want is None else want[1] - lo + 1)
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
    target = int(np.sort(h)[2])  # about three hits in the window
    want = first_index(h, lo, target)
    request.addfinalizer(lambda: engine.set_layout_policy(gpuhash.LAYOUT_AUTO))
    engine.set_layout_policy(policy)
    for rchunk in (0, 10):
        assert engine.first_below(m, lo, hi, target, rchunk=rchunk) == want, (name, mlen, d, rchunk)
        recs = engine.launches()
        if name == "tail":
            assert {(r["J"], r["digits"]) for r in recs} == {(j, d)}, recs
        else:
            assert any((r["C2"], r["J"]) == (c2, j) for r in recs), recs
        assert engine.stats()["nonces"] == want[1] - lo + 1
        assert engine.first_below(m, lo, hi, int(h.min()) - 1, rchunk=rchunk) is None


@pytest.mark.parametrize("m", [b"", b"bradfitz", M120[:50]], ids=["empty", "bradfitz", "two-blocks"])
def test_top_of_u64(engine, oracle, m):
    """A nonce of 2^64-1 is a legal answer: found is a flag, not a sentinel nonce."""
    lo = U64 - 4999
    h = oracle.hash_range(m, lo, 5000)
    # the longest suffix of the window whose strict minimum is at 2^64-1
    s = len(h) - 1
    while s > 0 and h[s - 1] > h[-1]:
        s -= 1
    target = int(h[-1])
    assert first_index(h[s:], lo + s, target) == (target, U64)
    assert engine.first_below(m, lo + s, U64, target) == (target, U64)
    assert engine.stats()["nonces"] == len(h) - s
    assert engine.first_below(m, lo + s, U64, target - 1) is None
    assert engine.first_below(m, U64, U64, target) == (target, U64)
    assert engine.first_below(m, U64, U64, U64) == (target, U64)
    assert engine.first_below(m, lo, U64, U64) == (int(h[0]), lo)


def test_shards(oracle):
    """Two contiguous shards (a context opened on [0, 0]): hits only in the upper shard, and
    hits in both; the lowest nonce wins either way."""
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
                want = first_index(h, lo, up_min)
                assert want[1] >= b0
                assert two.first_below(m, lo, hi, up_min) == want
            if "both" not in done:
                done.add("both")
                target = max(low_min, up_min)
                want = first_index(h, lo, target)
                assert want[1] < b0 and (h[b0 - lo:] <= np.uint64(target)).any()
                assert two.first_below(m, lo, hi, target) == want
                assert {r["shard"] for r in two.launches()} == {0, 1}
                assert two.stats()["ndevices"] == 2
            if done == {"upper", "both"}:
                break
        assert done == {"upper", "both"}
        assert two.first_below(m, lo, hi, min(low_min, up_min) - 1) is None


def test_slices_stop_after_the_first_hit(oracle, monkeypatch):
    """GPUHASH_SLICE_NONCES=50000 with the first hit in the third slice: the right answer,
    and no launch beyond that slice.  (A one-device context: a slice is 50,000 nonces per
    device.)"""
    import gpuhash
    monkeypatch.setenv("GPUHASH_SLICE_NONCES", "50000")
    m, size = b"bradfitz", 250_000
    for k in range(1, 40):
        lo = 7_000_000 + k * size
        h = oracle.hash_range(m, lo, size)
        target = int(h[100_000:150_000].min())
        if int(h[:100_000].min()) > target:
            break
    else:
        pytest.fail("no window with its first hit in the third slice")
    want = first_index(h, lo, target)
    assert lo + 100_000 <= want[1] < lo + 150_000
    with gpuhash.Engine([0]) as one:
        assert one.first_below(m, lo, lo + size - 1, target) == want
        recs = one.launches()
        assert {r["lo"] for r in recs} == {lo, lo + 50_000, lo + 100_000}, sorted({r["lo"] for r in recs})
        assert one.stats()["nonces"] == want[1] - lo + 1
        assert one.first_below(m, lo, lo + 99_999, target) is None
        assert {r["lo"] for r in one.launches()} == {lo, lo + 50_000}
        assert one.stats()["nonces"] == 100_000


def test_cli_below():
    out = subprocess.run([CLI, "--below", "bradfitz", "0", "9999", "1419516646206828"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "Result 1419516646206828 9898"
    out = subprocess.run([CLI, "--below", "bradfitz", "0", "9999", "1419516646206827"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "None", out.stderr
    out = subprocess.run([CLI, "--below", "bradfitz", "10", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "invalid argument" in out.stderr
    assert subprocess.run([CLI, "--below", "bradfitz", "0", "9999"], capture_output=True).returncode == 2


def test_early_exit(engine, golden):
    """A hit at nonce 9898 of [0, 2^34-1] ends the search early: eleven digit groups and
    several variant launches drain without hashing.  The golden says 9898 holds the minimum
    of [0, 9999], so it is the first nonce at or below that hash.  gpuhash_min over the same
    range, whose code this feature does not touch, is the yardstick; the expected ratio is
    around a hundredth, and a quarter is the condition that the search exits early at all."""
    g = next(r for r in golden["ranges"] if bytes.fromhex(r["msg_hex"]) == b"bradfitz"
             and (r["lower"], r["upper"]) == (0, 9999))
    assert (g["hash"], g["nonce"]) == (1419516646206828, 9898)
    hi = (1 << 34) - 1
    engine.first_below(b"bradfitz", 0, 99_999, g["hash"])  # warm-up: code objects, buffers
    t0 = time.perf_counter()
    got = engine.first_below(b"bradfitz", 0, hi, g["hash"])
    t_first = time.perf_counter() - t0
    st = engine.stats()
    t0 = time.perf_counter()
    engine.min(b"bradfitz", 0, hi)
    t_min = time.perf_counter() - t0
    print(f"first_below {t_first * 1e3:.2f} ms (kernel {st['kernel_ms']:.2f} ms, {st['launches']} launches), "
          f"min {t_min * 1e3:.2f} ms, ratio {t_first / t_min:.4f}")
    assert got == (1419516646206828, 9898)
    assert st["nonces"] == 9899
    assert t_first < t_min / 4, (t_first, t_min)
