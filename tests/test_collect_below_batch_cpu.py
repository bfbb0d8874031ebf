"""CPU: gpuhash_collect_below_batch -- many independent (message, lower, upper, target, room) hit
collections in one call, each counted and listed exactly as gpuhash_collect_below does it.

No GPU here: the ABI's exports and argument checks, the CPU replay of the kernel's collect batch
mode (hostcheck_collect_below_batch: the stage as fill() writes it, pieces in a seeded order with
several workgroups in flight, the job change, the per-job counters, the one shared list with its
64-bit append counter and its capacity, and the ENGINE's fold and re-runs, collect.h) against the
oracle, the code generation of the MODE 6 kernels, and a stand-alone sanitizer run of the replay.
Expected values come from oracle.hash_range + numpy (tests/collect_batch_jobs.py).
"""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import batch_jobs
import collect_batch_jobs
from collect_batch_jobs import answer
from test_codegen import kernel_metadata, pinned_runs
from test_collect_below_cpu import WINDOWS, window_hashes, window_msg
from test_min_batch_cpu import loop_bodies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
LLVM = "/opt/rocm/lib/llvm/bin"
U64 = (1 << 64) - 1
u64, u32, sz = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
AUTO, UNIFORM, CLASSIC, LANETABLE, TAIL_ALWAYS = 0, 1, 2, 3, 16
FUNCS = ("gpuhash_collect_below_batch", "gpuhash_collect_below_batch_ex")
MAX_JOBS, MAX_SPAN, COLLECT_MAX = 1 << 16, 1 << 38, 1 << 20
ORDERS = [0, 1, 12345, 987654321]  # ascending, a workgroup per piece (descending), two shuffles
BUFFERS = [8, 64, 1 << 20]
MARK = 0xDEADBEEF
NEW_OBJECTS = ("kernels_plain_collectbatch", "kernels_ut_collectbatch", "kernels_misc_collectbatch")


# ---- 1. exports and checks ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_collect_below_batch(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", src), f
        assert f in exported, f  # unmangled extern "C"
        assert hasattr(lib, f)
    import gpuhash
    assert set(FUNCS) <= set(gpuhash.EXPORTED)
    assert hasattr(gpuhash.Engine, "collect_below_batch") and hasattr(gpuhash.Engine, "count_below_batch")


def test_version_is_at_least_0_8(lib):
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 8)


def test_collect_below_batch_argument_errors_need_no_device(lib):
    import gpuhash
    EINVAL, ETOOLONG = gpuhash.GPUHASH_EINVAL, gpuhash.GPUHASH_ETOOLONG
    f, fx = lib.gpuhash_collect_below_batch, lib.gpuhash_collect_below_batch_ex
    msgs = ctypes.create_string_buffer(b"abcdef")
    mp = ctypes.addressof(msgs)
    off = (sz * 3)(0, 3, 6)
    lo, hi, tg = (u64 * 2)(0, 5), (u64 * 2)(9, 5), (u64 * 2)(U64, U64)
    oo = (sz * 3)(0, 2, 4)
    x, h, tt = (u64 * 4)(7, 7, 7, 7), (u64 * 4)(7, 7, 7, 7), (u64 * 2)(7, 7)
    garbage = ctypes.create_string_buffer(b"\xA5" * 64, 64)  # not a context: never read as one

    def both(want, ctx_, mp_, off_, nj, lo_, hi_, tg_, oo_, x_, h_, tt_):
        assert f(ctx_, mp_, off_, nj, lo_, hi_, tg_, oo_, x_, h_, tt_) == want
        assert fx(ctx_, mp_, off_, nj, lo_, hi_, tg_, 7, oo_, x_, h_, tt_) == want

    both(EINVAL, None, mp, off, 2, lo, hi, tg, oo, x, h, tt)     # null pointers, one at a time
    for ctx in (ctypes.c_void_p(1), ctypes.c_void_p(ctypes.addressof(garbage))):
        both(EINVAL, ctx, None, off, 2, lo, hi, tg, oo, x, h, tt)    # (non-empty messages need msgs)
        both(EINVAL, ctx, mp, None, 2, lo, hi, tg, oo, x, h, tt)
        both(EINVAL, ctx, mp, off, 2, None, hi, tg, oo, x, h, tt)
        both(EINVAL, ctx, mp, off, 2, lo, None, tg, oo, x, h, tt)
        both(EINVAL, ctx, mp, off, 2, lo, hi, None, oo, x, h, tt)    # target
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, oo, x, h, None)    # out_totals
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, None, x, h, None)  # ... for a pure count too
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, oo, None, h, tt)   # room asked with a null array
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, oo, x, None, tt)
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, (sz * 3)(0, 3, 2), x, h, tt)              # out_off decreases
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, (sz * 3)(0, 1, COLLECT_MAX + 2), x, h, tt)  # cap_1 = MAX + 1
        both(EINVAL, ctx, mp, off, 0, lo, hi, tg, oo, x, h, tt)      # njobs == 0
        big = MAX_JOBS + 1                                           # njobs > GPUHASH_BATCH_MAX_JOBS
        both(EINVAL, ctx, mp, (sz * (big + 1))(), big, (u64 * big)(), (u64 * big)(), (u64 * big)(), None, None, None,
             (u64 * big)())
        both(EINVAL, ctx, mp, (sz * 3)(0, 4, 3), 2, lo, hi, tg, oo, x, h, tt)          # msg_off decreases
        both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 6), hi, tg, oo, x, h, tt)           # lower[1] > upper[1]
        both(EINVAL, ctx, mp, off, 2, lo, (u64 * 2)(9, 5 + MAX_SPAN), tg, oo, x, h, tt)  # a span above the maximum
        both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 0), (u64 * 2)(9, U64), tg, oo, x, h, tt)
        long_off = (sz * 3)(0, 3, 3 + gpuhash.GPUHASH_MAX_MSG + 1)                     # a message over GPUHASH_MAX_MSG
        both(ETOOLONG, ctx, mp, long_off, 2, lo, hi, tg, oo, x, h, tt)                 #   (its bytes are never read)
        both(EINVAL, ctx, mp, long_off, 2, (u64 * 2)(0, 6), hi, tg, oo, x, h, tt)      # ... an EINVAL elsewhere comes first
        # a null out_off with null arrays is no error: the checks go on to the last of them
        both(ETOOLONG, ctx, mp, long_off, 2, lo, hi, tg, None, None, None, tt)
    assert list(x) == [7] * 4 and list(h) == [7] * 4 and list(tt) == [7, 7]  # nothing written
    assert garbage.raw == b"\xA5" * 64


def test_binding_refuses_bad_jobs_before_calling_in():
    import gpuhash
    eng = gpuhash.Engine.__new__(gpuhash.Engine)  # no context: the checks come first
    eng._ctx = None
    for jobs in ([], [(b"x", 5, 4, 0)], [(b"x", 0, 4, 0), (b"y", -1, 4, 0)], [(b"x", 0, 1 << 64, 0)],
                 [(b"x", 0, MAX_SPAN, 0)], [(b"x", 0, 4)], [(b"x", 0, 4, 1 << 64)], [(b"x", 0, 4, -1)],
                 [(bytes(gpuhash.GPUHASH_MAX_MSG + 1), 0, 1, 0)], [(b"x", 0, 4, 0, -1)],
                 [(b"x", 0, 4, 0, COLLECT_MAX + 1)], [(b"x", 0, 4, 0, 1, 1)]):
        with pytest.raises(ValueError):
            eng.collect_below_batch(jobs)
    for jobs in ([], [(b"x", 5, 4, 0)], [(b"x", 0, 4)], [(b"x", 0, 4, 0, 1)], [(b"x", 0, 4, 1 << 64)]):
        with pytest.raises(ValueError):
            eng.count_below_batch(jobs)
    for jobs in ([(b"x", 0.0, 4, 0)], [(b"x", 0, 4, 0.5)], [(b"x", 0, 4, 0, 1.0)], [(b"x", 0, 4, 0, True)]):
        with pytest.raises(TypeError):
            eng.collect_below_batch(jobs)
    with pytest.raises(ValueError):
        eng.collect_below_batch([(b"x", 0, 4, 0)], rchunk=-1)


# ---- 2. the replay against the oracle ----

@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.hostcheck_collect_below_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int,
                                                  u64, vp, vp, vp, vp, vp]
    return lib


def replay(hc, jobs, rchunk=0, policy=AUTO, order=0, batch_bytes=0, nshards=1, buffer=COLLECT_MAX, count_only=False):
    """hostcheck_collect_below_batch over (message, lower, upper, target, cap) jobs: ([(total, hits)],
    info), info = (largest list fill of a run, jobs re-run, sub-batches, sub-range runs of the
    re-runs).  Entries from min(cap, total) on must be left untouched.  count_only passes a null
    out_off and null arrays."""
    msgs, off, lower, upper, target, out_off = collect_batch_jobs.flat(jobs)
    room = int(out_off[-1])
    x = np.full(max(room, 1), MARK, dtype=np.uint64)
    h = np.full(max(room, 1), MARK, dtype=np.uint64)
    totals = np.full(len(jobs), MARK, dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    outs = (None, None, None) if count_only else (out_off.ctypes.data, x.ctypes.data, h.ctypes.data)
    rc = hc.hostcheck_collect_below_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data,
                                          upper.ctypes.data, target.ctypes.data, rchunk, policy, order, batch_bytes,
                                          nshards, buffer, *outs, totals.ctypes.data, info.ctypes.data)
    assert rc == 0  # -3: the list and the counters disagree
    got = []
    for k, j in enumerate(jobs):
        at, cap = int(out_off[k]), 0 if count_only else j[4]
        held = min(cap, int(totals[k]))
        assert (x[at + held:at + cap] == MARK).all() and (h[at + held:at + cap] == MARK).all(), k
        got.append((int(totals[k]), [(int(h[at + i]), int(x[at + i])) for i in range(held)]))
    if count_only:
        assert (x == MARK).all() and (h == MARK).all()
    return got, tuple(int(v) for v in info)


@pytest.fixture(scope="module")
def mix(oracle):
    """The job mix with its targets and rooms, and the oracle's answers."""
    return collect_batch_jobs.jobs_and_answers(oracle)


def test_the_jobs_are_what_the_issue_asks_for(mix):
    jobs, want = mix
    assert [j[:3] for j in jobs] == [(m, a, b) for _, m, a, b in batch_jobs.job_mix()]
    assert 150 <= len(jobs) <= 250 and max(b - a + 1 for _, a, b, _, _ in jobs) <= 5000
    assert [j[4] for j in jobs] == [(0, 5, 5000)[k % 3] for k in range(len(jobs))]
    kinds = [k % 5 for k in range(len(jobs))]
    assert all(w[0] == 0 for w, k in zip(want, kinds) if k == 0)
    assert all(w[0] >= 1 for w, k in zip(want, kinds) if k == 1)
    assert all(t == U64 and w[0] == b - a + 1 for (_, a, b, t, _), w, k in zip(jobs, want, kinds) if k == 4)
    # the 2^64-1 jobs alone hold thousands of hits; some list fewer than they count, some all
    assert sum(w[0] for (_, _, _, t, cap), w in zip(jobs, want) if t == U64 and cap) > 5000
    assert any(len(w[1]) == 5 < w[0] for w in want) and any(len(w[1]) == w[0] > 64 for w in want)
    assert any(j[2] == U64 and w[0] for j, w in zip(jobs, want))  # a hit at the top of uint64


@pytest.mark.parametrize("buffer", BUFFERS)
@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_replay_matches_the_oracle(hc, mix, policy, rchunk, buffer):
    jobs, want = mix
    for order in ORDERS:
        got, info = replay(hc, jobs, rchunk, policy, order, buffer=buffer)
        bad = [(k, jobs[k][1:], g[0], w[0]) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (order, bad[:3])
        assert info[0] <= buffer and info[2] == 1, (order, info)
        if buffer < COLLECT_MAX:  # the overflow and re-run path ran
            assert info[0] == buffer and info[1] > 0 and info[3] > info[1], (order, info)
        else:
            # a listing job appends every hit, whatever its room; nothing is re-run
            assert info[1] == 0 and info[3] == 0 and info[0] == sum(w[0] for j, w in zip(jobs, want) if j[4]), (order, info)


def test_only_jobs_the_list_cut_short_are_re_run(hc, mix):
    """A list that holds every hit of the listing jobs but one entry: one job at least is re-run,
    never a count-only one, and the answers do not change."""
    jobs, want = mix
    listed = sum(w[0] for j, w in zip(jobs, want) if j[4])
    got, info = replay(hc, jobs, order=12345, buffer=listed - 1)
    assert got == want and info[0] == listed - 1 and 1 <= info[1] <= sum(1 for j in jobs if j[4])
    got, info = replay(hc, jobs, order=12345, buffer=listed)
    assert got == want and info[:2] == (listed, 0)


def test_permuting_the_jobs_permutes_the_results(hc, mix):
    jobs, want = mix
    perm = list(range(len(jobs)))
    random.Random("collect-below-batch permutation").shuffle(perm)
    for order, buffer in ((0, COLLECT_MAX), (987654321, 64)):
        got, _ = replay(hc, [jobs[i] for i in perm], 0, AUTO, order, buffer=buffer)
        assert got == [want[i] for i in perm]
    back = list(reversed(range(len(jobs))))
    got, _ = replay(hc, [jobs[i] for i in back], 7, LANETABLE, 1, buffer=8)
    assert got == [want[i] for i in back]


def test_sub_batches_and_entry_runs_do_not_change_the_results(hc, mix, monkeypatch):
    jobs, want = mix
    small = 256 * 1024
    for policy, order, buffer in ((AUTO, 0, COLLECT_MAX), (LANETABLE, 12345, 64)):
        got, info = replay(hc, jobs, 0, policy, order, batch_bytes=small, buffer=buffer)
        assert got == want and info[2] >= 3, info
    for nshards in (1, 2, 3):
        for buffer in (COLLECT_MAX, 64):
            got, info = replay(hc, jobs, 0, AUTO, 12345, nshards=nshards, buffer=buffer)
            assert got == want and info[2] == 1, (nshards, buffer, info)
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", str(small))  # the override the engine reads
    got, info = replay(hc, jobs, 7, AUTO, 1, nshards=2, buffer=8)
    assert got == want and info[2] >= 3, info
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", "1")  # every job a sub-batch of its own
    got, info = replay(hc, jobs[:40], 0, AUTO, 0)
    assert got == want[:40] and info[2] == 40


# ---- 3. jobs do not share state ----

def test_twenty_targets_over_one_range_give_twenty_answers(hc, oracle):
    name, mlen, policy, lo, cnt, _ = WINDOWS[0]
    m = window_msg(name, mlen)
    h = window_hashes(oracle, name, m, lo, cnt)
    s = np.sort(h)
    ranks = [0, 1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63, 94, 141, 211, 316, 474, 711, 1066, 1599]
    targets = [int(s[r]) for r in ranks]  # from the least hash upward, ever denser
    jobs = [(m, lo, lo + cnt - 1, t, (2000, 0, 7)[k % 3]) for k, t in enumerate(targets)]
    want = [answer(h, lo, t, cap) for _, _, _, t, cap in jobs]
    assert len({w[0] for w in want}) == 20  # really different answers: the counters are per job
    for order in ORDERS:
        for buffer in (COLLECT_MAX, 64):
            assert replay(hc, jobs, 0, policy, order, buffer=buffer)[0] == want, (order, buffer)
    # and two jobs of one message with overlapping ranges
    half = lo + cnt // 2
    jobs = [(m, lo, half + 500, targets[9], 100), (m, half - 500, lo + cnt - 1, targets[9], 100), (m, lo, lo + cnt - 1, 0, 9)]
    want = [answer(h[:half + 501 - lo], lo, targets[9], 100), answer(h[half - 500 - lo:], half - 500, targets[9], 100),
            (0, [])]
    assert replay(hc, jobs, 7, policy, 12345)[0] == want


def test_a_count_only_batch_appends_nothing(hc, mix):
    jobs, want = mix
    for order, buffer in ((0, COLLECT_MAX), (12345, 8)):
        got, info = replay(hc, jobs, 0, AUTO, order, buffer=buffer, count_only=True)
        assert got == [(w[0], []) for w in want]
        assert info[0] == 0 and info[1] == 0 and info[3] == 0, info  # no entry, no re-run


# ---- 4. code generation of the MODE 6 kernels ----

def _tools():
    return shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))


def test_plain_collect_batch_kernels_fit_8_waves_and_keep_the_loop(tmp_path):
    """J = 4 and J = 13: 64 VGPRs at most and no spill, one per-nonce loop with MODE 0's VALU work
    (1,196 and 1,038 instructions; the build has 1,196 and 1,037, one fewer at J = 13) opening at
    the code phase MODE 4's loop of the same J opens at.  Every other plain J spills no more than
    MODE 3's kernel of the same J, as tests/golden/kernel_manifest.txt records it."""
    if not _tools():
        pytest.skip("binutils / ROCm LLVM tools not present")
    objs, dirs = {}, {}
    for tu in ("kernels_plain_collectbatch", "kernels_plain_batch", "kernels_plain"):
        objs[tu] = os.path.join(PKG, "build", tu + ".o")
        if not os.path.exists(objs[tu]):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{tu}.o"])
        dirs[tu] = tmp_path / tu
        dirs[tu].mkdir()
    meta = kernel_metadata(objs["kernels_plain_collectbatch"], dirs["kernels_plain_collectbatch"])
    scans = {}
    for name, v in meta.items():
        m = re.search(r"k_scanILi(\d+)ELi0ELb0ELi6E", name)  # MODE 6
        if m:
            scans[int(m.group(1))] = v
    assert sorted(scans) == list(range(14)), scans
    for J in (4, 13):
        assert scans[J][0] <= 64 and scans[J][1] == 0, (J, scans[J])
    mode3 = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.txt")).read().splitlines():
        m = re.search(r"^kernels_plain_collect\.o \S*k_scanILi(\d+)ELi0ELb0ELi3E\S* .*vgpr_spill_count=(\d+)", line)
        if m:
            mode3[int(m.group(1))] = int(m.group(2))
    assert sorted(mode3) == list(range(14)), mode3
    for J, (vgpr, spill) in scans.items():
        assert vgpr <= 64 and spill <= mode3[J], (J, vgpr, spill, mode3[J])
    kernel_metadata(objs["kernels_plain_batch"], dirs["kernels_plain_batch"])
    kernel_metadata(objs["kernels_plain"], dirs["kernels_plain"])
    for J, valu in ((4, 1196), (13, 1038)):
        name = "_ZN7gpuhash6k_scanILi%dELi0ELb0ELi%dEE"
        mine = loop_bodies(dirs["kernels_plain_collectbatch"] / "k.co", name % (J, 6))
        plain = loop_bodies(dirs["kernels_plain"] / "k.co", name % (J, 0))
        assert len(mine) == 1 and len(plain) == 1 and plain[0][1] == valu, (J, mine, plain)
        assert mine[0][1] <= valu, (J, mine, plain)
        pins = [p for p in pinned_runs(dirs["kernels_plain_collectbatch"] / "k.co", name % (J, 6)) if p is not None]
        theirs = [p for p in pinned_runs(dirs["kernels_plain_batch"] / "k.co", name % (J, 4)) if p is not None]
        assert len(pins) == 1 and len(theirs) == 1 and pins[0] % 8 == theirs[0] % 8 == 4, (J, pins, theirs)


def test_every_collect_batch_kernel_is_the_recorded_one():
    """Every kernel of the three MODE 6 objects against tests/golden/kernel_manifest_collect_batch.txt,
    as tests/test_codegen.py holds the other 129 against kernel_manifest.txt: a layout for every
    layout MODE 0 has.  After an intended kernel change or a compiler update, regenerate it:
    python tools/kernel_manifest.py bitcoin-miner_amd/build/kernels_{plain,ut,misc}_collectbatch.o"""
    if not _tools():
        pytest.skip("binutils / ROCm LLVM tools not present")
    golden = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "kernel_manifest_collect_batch.txt")).read().splitlines():
        obj, sym, rest = line.split(" ", 2)
        golden[obj, sym] = rest
    assert sorted({obj for obj, _ in golden}) == sorted(o + ".o" for o in NEW_OBJECTS)
    missing = [f"build/{o}.o" for o in NEW_OBJECTS if not os.path.exists(os.path.join(PKG, "build", o + ".o"))]
    if missing:
        subprocess.check_call(["make", "-s", "-j8", "-C", PKG] + missing)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_manifest.py")]
                                  + [os.path.join(PKG, "build", o + ".o") for o in NEW_OBJECTS], text=True)
    built = {}
    for line in out.splitlines():
        obj, sym, rest = line.split(" ", 2)
        built[obj, sym] = rest
    assert sorted(built) == sorted(golden), sorted(set(built) ^ set(golden))
    differ = [f"{obj} {sym}" for (obj, sym), rest in sorted(golden.items()) if built[obj, sym] != rest]
    assert not differ, f"{len(differ)} kernels differ from the fixture:\n" + "\n".join(differ)
    # MODE 6 of every layout MODE 0 is built for
    def layouts(symbols, mode):
        found = (re.search(r"k_scanILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE", s) for s in symbols)
        return sorted(m.groups()[:3] for m in found if m and int(m.group(4)) == mode)
    recorded = [line.split(" ", 2)[1] for line in
                open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.txt")).read().splitlines()]
    assert layouts([s for _, s in golden], 6) == layouts(recorded, 0) and len(golden) == 21


# ---- 5. sanitizers ----

def test_collect_batch_replay_stand_alone_under_asan_ubsan():
    """A program with its own main over hostcheck_collect_below_batch (csrc/hostcheck_collectbatch_main.cpp),
    built with -fsanitize=address,undefined: 330 jobs with every kind of target and room under
    every policy, lists of 1, 8, 64, 1000 and 2^20 entries, sub-batches down to one job each, three
    context entries, count-only batches and the top of uint64; each job checked against an
    ascending scan."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/hostcheck_collectbatch_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIBDIR, "hostcheck_collectbatch_asan")], env=env, capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.strip() == "ok", out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
