"""CPU: gpuhash_first_below_batch -- many independent (message, lower, upper, target) first-hit
searches in one call, each answered exactly as gpuhash_first_below answers it.

No GPU here: the ABI's exports and argument checks, the CPU replay of the kernel's first-hit batch
mode (hostcheck_first_below_batch: the stage as fill() writes it, its groups in ascending digit
order, pieces in a seeded order with several workgroups in flight, the job-change flush, the bound
read at a grab and at a job change, the skip and drain rules, the result list with its bound)
against the oracle, the stage's layout and order, the order's property (a job whose answer has d
digits never hashes a nonce of more than d digits), the code generation of the MODE 5 plain
kernels, and a stand-alone sanitizer run of the replay.  Expected values come from
oracle.hash_range + numpy (tests/first_batch_jobs.py).
"""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_jobs
import first_batch_jobs
from first_batch_jobs import first_index
from test_codegen import kernel_metadata, pinned_runs
from test_collect_below_cpu import WINDOWS, window_hashes, window_msg
from test_min_batch_cpu import DESC_BYTES, DESC_JOB, EXTRA, FIELDS, LIST_HEAD, descriptors, loop_bodies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
LLVM = "/opt/rocm/lib/llvm/bin"
U64 = (1 << 64) - 1
u64, u32, sz = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
pu64 = ctypes.POINTER(u64)
AUTO, UNIFORM, CLASSIC, LANETABLE, TAIL_ALWAYS = 0, 1, 2, 3, 16
FUNCS = ("gpuhash_first_below_batch", "gpuhash_first_below_batch_ex")
MAX_JOBS, MAX_SPAN = 1 << 16, 1 << 38
ORDERS = [0, 1, 12345, 987654321]  # ascending, descending, two shuffles
MARK = 0xDEADBEEF
# 32-bit word positions in LaunchDesc (plan.h): p_first, r_first, base (64-bit), stride, tail
DESC_R, DESC_P_FIRST, DESC_R_FIRST, DESC_BASE, DESC_STRIDE, DESC_TAIL = 132, 135, 137, 142, 145, 146


# ---- 1. exports and checks ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_first_below_batch(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", src), f
        assert f in exported, f  # unmangled extern "C"
        assert hasattr(lib, f)
    import gpuhash
    assert set(FUNCS) <= set(gpuhash.EXPORTED)
    assert hasattr(gpuhash.Engine, "first_below_batch")


def test_version_is_at_least_0_7(lib):
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 7)


def test_first_below_batch_argument_errors_need_no_device(lib):
    import gpuhash
    EINVAL, ETOOLONG = gpuhash.GPUHASH_EINVAL, gpuhash.GPUHASH_ETOOLONG
    f, fx = lib.gpuhash_first_below_batch, lib.gpuhash_first_below_batch_ex
    msgs = ctypes.create_string_buffer(b"abcdef")
    mp = ctypes.addressof(msgs)
    off = (sz * 3)(0, 3, 6)
    lo, hi, tg = (u64 * 2)(0, 5), (u64 * 2)(9, 5), (u64 * 2)(U64, U64)
    h, n, fd = (u64 * 2)(7, 7), (u64 * 2)(7, 7), (ctypes.c_int * 2)(7, 7)
    garbage = ctypes.create_string_buffer(b"\xA5" * 64, 64)  # not a context: never read as one

    def both(want, ctx_, mp_, off_, nj, lo_, hi_, tg_, h_, n_, fd_):
        assert f(ctx_, mp_, off_, nj, lo_, hi_, tg_, h_, n_, fd_) == want
        assert fx(ctx_, mp_, off_, nj, lo_, hi_, tg_, 7, h_, n_, fd_) == want

    both(EINVAL, None, mp, off, 2, lo, hi, tg, h, n, fd)     # null pointers, one at a time
    for ctx in (ctypes.c_void_p(1), ctypes.c_void_p(ctypes.addressof(garbage))):
        both(EINVAL, ctx, None, off, 2, lo, hi, tg, h, n, fd)    # (non-empty messages need msgs)
        both(EINVAL, ctx, mp, None, 2, lo, hi, tg, h, n, fd)
        both(EINVAL, ctx, mp, off, 2, None, hi, tg, h, n, fd)
        both(EINVAL, ctx, mp, off, 2, lo, None, tg, h, n, fd)
        both(EINVAL, ctx, mp, off, 2, lo, hi, None, h, n, fd)    # target
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, None, n, fd)
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, h, None, fd)
        both(EINVAL, ctx, mp, off, 2, lo, hi, tg, h, n, None)    # out_found
        both(EINVAL, ctx, mp, off, 0, lo, hi, tg, h, n, fd)      # njobs == 0
        big = MAX_JOBS + 1                                       # njobs > GPUHASH_BATCH_MAX_JOBS
        both(EINVAL, ctx, mp, (sz * (big + 1))(), big, (u64 * big)(), (u64 * big)(), (u64 * big)(), (u64 * big)(),
             (u64 * big)(), (ctypes.c_int * big)())
        both(EINVAL, ctx, mp, (sz * 3)(0, 4, 3), 2, lo, hi, tg, h, n, fd)          # msg_off decreases
        both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 6), hi, tg, h, n, fd)           # lower[1] > upper[1]
        both(EINVAL, ctx, mp, off, 2, lo, (u64 * 2)(9, 5 + MAX_SPAN), tg, h, n, fd)  # a span above the maximum
        both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 0), (u64 * 2)(9, U64), tg, h, n, fd)
        long_off = (sz * 3)(0, 3, 3 + gpuhash.GPUHASH_MAX_MSG + 1)                 # a message over GPUHASH_MAX_MSG
        both(ETOOLONG, ctx, mp, long_off, 2, lo, hi, tg, h, n, fd)                 #   (its bytes are never read)
        both(EINVAL, ctx, mp, long_off, 2, (u64 * 2)(0, 6), hi, tg, h, n, fd)      # ... an EINVAL elsewhere comes first
    assert list(h) == [7, 7] and list(n) == [7, 7] and list(fd) == [7, 7]  # nothing written
    assert garbage.raw == b"\xA5" * 64


def test_binding_refuses_bad_jobs_before_calling_in():
    import gpuhash
    eng = gpuhash.Engine.__new__(gpuhash.Engine)  # no context: the checks come first
    eng._ctx = None
    for jobs in ([], [(b"x", 5, 4, 0)], [(b"x", 0, 4, 0), (b"y", -1, 4, 0)], [(b"x", 0, 1 << 64, 0)],
                 [(b"x", 0, MAX_SPAN, 0)], [(b"x", 0, 4)], [(b"x", 0, 4, 1 << 64)], [(b"x", 0, 4, -1)],
                 [(bytes(gpuhash.GPUHASH_MAX_MSG + 1), 0, 1, 0)]):
        with pytest.raises(ValueError):
            eng.first_below_batch(jobs)
    with pytest.raises(TypeError):
        eng.first_below_batch([(b"x", 0.0, 4, 0)])
    with pytest.raises(TypeError):
        eng.first_below_batch([(b"x", 0, 4, 0.5)])
    with pytest.raises(ValueError):
        eng.first_below_batch([(b"x", 0, 4, 0)], rchunk=-1)


# ---- 2. the replay against the oracle ----

@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_first_below_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int,
                                                vp, vp, vp, vp, vp]
    lib.hostcheck_stage_first_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, vp, ctypes.c_int, pu64, vp, vp, u64]
    lib.hostcheck_stage.argtypes = [ctypes.c_char_p, u64, u64, u64, u32, pu64, ctypes.c_int, pu64, vp, u64]
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


def replay(hc, jobs, rchunk=0, policy=AUTO, order=0, batch_bytes=0, nshards=1):
    """hostcheck_first_below_batch over (message, lower, upper, target) jobs: ([(hash, nonce) or
    None], [(hashed, largest hashed, hashed from lower to the answer)], fill), fill = (largest list
    fill of a run, that run's bound, runs over their bound, sub-batches).  A job that is not found
    must leave its outputs untouched."""
    msgs, off, lower, upper, target = first_batch_jobs.flat(jobs)
    h = np.full(len(jobs), MARK, dtype=np.uint64)
    n = np.full(len(jobs), MARK, dtype=np.uint64)
    found = np.full(len(jobs), -1, dtype=np.int32)
    trace = np.zeros((len(jobs), 3), dtype=np.uint64)
    fill = np.zeros(4, dtype=np.uint64)
    rc = hc.hostcheck_first_below_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data,
                                        upper.ctypes.data, target.ctypes.data, rchunk, policy, order, batch_bytes,
                                        nshards, h.ctypes.data, n.ctypes.data, found.ctypes.data, trace.ctypes.data,
                                        fill.ctypes.data)
    assert rc == 0  # -2: a nonce was hashed twice
    assert set(found.tolist()) <= {0, 1}
    got = []
    for k in range(len(jobs)):
        if found[k]:
            got.append((int(h[k]), int(n[k])))
        else:
            assert (int(h[k]), int(n[k])) == (MARK, MARK)
            got.append(None)
    return got, [tuple(int(v) for v in row) for row in trace], tuple(int(v) for v in fill)


@pytest.fixture(scope="module")
def mix(oracle):
    """The job mix with its targets, and the oracle's answers."""
    return first_batch_jobs.jobs_and_answers(oracle)


def check_trace(jobs, got, trace):
    """The order's property and the two completeness rules, for every job."""
    for (m, a, b, t), g, (hashed, largest, upto) in zip(jobs, got, trace):
        if g is None:
            assert hashed == b - a + 1, (a, b, t, hashed)
        else:
            assert len(str(largest)) <= len(str(g[1])), (a, b, t, g, largest)
            assert upto == g[1] - a + 1 <= hashed, (a, b, t, g, upto, hashed)


def test_the_jobs_are_what_the_issue_asks_for(mix):
    jobs, want = mix
    assert [j[:3] for j in jobs] == [(m, a, b) for _, m, a, b in batch_jobs.job_mix()]
    assert 150 <= len(jobs) <= 250 and max(b - a + 1 for _, a, b, _ in jobs) <= 5000
    kinds = [k % first_batch_jobs.KINDS for k in range(len(jobs))]
    assert all(t == 0 for (_, _, _, t), k in zip(jobs, kinds) if k == 0)
    assert all(t == U64 and w[1] == a for (_, a, _, t), w, k in zip(jobs, want, kinds) if k == 1)
    assert all(w is not None and w[0] == t for (_, _, _, t), w, k in zip(jobs, want, kinds) if k == 2)
    assert all(w is None for w, k in zip(want, kinds) if k in (0, 4))  # no hash of the mix is 0
    found = [w for w in want if w is not None]
    assert len(found) > len(jobs) // 2 and any(w[1] == U64 for w in found)
    # answers that are not at `lower`, and answers in a lower digit count than `upper`
    assert sum(w[1] != a for (_, a, _, _), w in zip(jobs, want) if w) >= 20
    assert sum(len(str(w[1])) < len(str(b)) for (_, _, b, _), w in zip(jobs, want) if w) >= 5


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_replay_matches_the_oracle(hc, mix, policy, rchunk):
    jobs, want = mix
    for order in ORDERS:
        got, trace, fill = replay(hc, jobs, rchunk, policy, order)
        bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (order, bad[:3])
        assert fill[2] == 0 and 0 < fill[0] <= fill[1] and fill[3] == 1, (order, fill)
        check_trace(jobs, got, trace)


def test_replay_over_several_entries(hc, mix):
    jobs, want = mix
    for order in (0, 12345):
        got, trace, fill = replay(hc, jobs, 0, AUTO, order, nshards=3)
        assert got == want and fill[2] == 0
        check_trace(jobs, got, trace)


def test_permuting_the_jobs_permutes_the_results(hc, mix):
    jobs, want = mix
    perm = list(range(len(jobs)))
    random.Random("first-below-batch permutation").shuffle(perm)
    for order in (0, 987654321):
        got, _, _ = replay(hc, [jobs[i] for i in perm], 0, AUTO, order)
        assert got == [want[i] for i in perm]
    back = list(reversed(range(len(jobs))))
    got, _, _ = replay(hc, [jobs[i] for i in back], 7, LANETABLE, 1)
    assert got == [want[i] for i in back]


def test_sub_batches_do_not_change_the_results(hc, mix, monkeypatch):
    jobs, want = mix
    small = 256 * 1024
    for policy, order in ((AUTO, 0), (LANETABLE, 12345)):
        got, trace, fill = replay(hc, jobs, 0, policy, order, batch_bytes=small)
        assert got == want and fill[3] >= 3 and fill[2] == 0, fill
        check_trace(jobs, got, trace)
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", str(small))  # the override the engine reads
    got, _, fill = replay(hc, jobs, 7, AUTO, 1, nshards=2)
    assert got == want and fill[3] >= 3 and fill[2] == 0, fill
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", "1")  # every job a sub-batch of its own
    got, _, fill = replay(hc, jobs[:40], 0, AUTO, 0)
    assert got == want[:40] and fill[3] == 40


# ---- 3. jobs do not share state ----

def test_twenty_targets_over_one_range_give_twenty_answers(hc, oracle):
    name, mlen, policy, lo, cnt, _ = WINDOWS[0]
    m = window_msg(name, mlen)
    h = window_hashes(oracle, name, m, lo, cnt)
    s = np.sort(h)
    ranks = [0, 1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63, 94, 141, 211, 316, 474, 711, 1066, 1599]
    targets = [int(s[r]) for r in ranks]  # from the least hash upward, ever denser
    jobs = [(m, lo, lo + cnt - 1, t) for t in targets]
    want = [first_index(h, lo, t) for t in targets]
    assert len({w[1] for w in want}) >= 5  # really different answers
    for order in ORDERS:
        got, trace, _ = replay(hc, jobs, 0, policy, order)
        assert got == want, order
        check_trace(jobs, got, trace)
    # and two jobs of one message with overlapping ranges
    half = lo + cnt // 2
    jobs = [(m, lo, half + 500, targets[3]), (m, half - 500, lo + cnt - 1, targets[3]), (m, lo, lo + cnt - 1, 0)]
    want = [first_index(h[:half + 501 - lo], lo, targets[3]), first_index(h[half - 500 - lo:], half - 500, targets[3]),
            None]
    assert replay(hc, jobs, 7, policy, 12345)[0] == want


# ---- 4. the stage ----

def stage_first(hc, jobs, rchunk=0):
    """(groups as dicts of FIELDS in launch order, extra as a dict of EXTRA, the metadata buffer)."""
    msgs, off, lower, upper, target = first_batch_jobs.flat(jobs)
    out = np.zeros((256, len(FIELDS)), dtype=np.uint64)
    extra = np.zeros(8, dtype=np.uint64)
    size = u64()
    args = (msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data, upper.ctypes.data, target.ctypes.data,
            rchunk, out.ctypes.data, 256, ctypes.byref(size), extra.ctypes.data)
    n = hc.hostcheck_stage_first_batch(*args, None, 0)
    assert 0 < n <= 256
    meta = np.zeros(size.value // 8, dtype=np.uint64)
    assert hc.hostcheck_stage_first_batch(*args, meta.ctypes.data, meta.nbytes) == n and size.value == meta.nbytes
    return ([dict(zip(FIELDS, (int(v) for v in row))) for row in out[:n]],
            dict(zip(EXTRA, (int(v) for v in extra))), meta.view(np.uint8))


def first_nonce(w):
    """The lowest nonce of a descriptor of a layout other than the lane table (plan.h)."""
    base = int(w[DESC_BASE]) | int(w[DESC_BASE + 1]) << 32
    return ((base + int(w[DESC_P_FIRST]) * int(w[DESC_R]) + int(w[DESC_R_FIRST])) * int(w[DESC_STRIDE])
            + int(w[DESC_TAIL])) & U64


def test_stage_groups_by_digits_ascending(hc, mix):
    jobs, _ = mix
    for policy in batch_jobs.POLICIES:
        hc.hostcheck_set_layout_policy(policy)
        groups, extra, meta = stage_first(hc, jobs)
        keys = [(g["d"], g["J"], g["C2"], g["EX"]) for g in groups]
        assert len(set(keys)) == len(keys)                  # keyed (d, J, C2, EX)
        assert [k[0] for k in keys] == sorted(k[0] for k in keys)  # d never decreases along the launches
        assert len(set(k[1:] for k in keys)) < len(keys)    # more launches than variants: that is the cost
        regions = [(0, 40 * len(groups))]
        for g in groups:
            words = descriptors(meta, g)
            job = words[:, DESC_JOB].astype(np.int64)
            assert (np.diff(job) >= 0).all() and job.max() < len(jobs)  # jobs ascend, each one's contiguous
            if g["C2"] != 3:  # every descriptor of the group has the group's digit count
                assert all(len(str(first_nonce(w))) == g["d"] for w in words), keys
            offs = meta[g["offs_at"]:g["offs_at"] + 8 * (g["ndesc"] + 1)].view(np.uint64).tolist()
            rows = [((int(w[136]) - int(w[135])) // 256 + 1) * int(w[DESC_R]) for w in words]
            assert offs == [sum(rows[:k]) for k in range(len(rows) + 1)] and g["total"] == offs[-1]
            regions += [(g["offs_at"], 8 * (g["ndesc"] + 1)), (g["desc_at"], g["desc_bytes"]),
                        (g["ptab_at"], g["ptab_bytes"])]
        # the per-job region: 16 bytes per job, armed {all ones, target[k]}
        assert extra["thresh_bytes"] == 16 * len(jobs)
        pairs = meta[extra["thresh_at"]:extra["thresh_at"] + extra["thresh_bytes"]].view(np.uint64).reshape(-1, 2)
        assert (pairs[:, 0] == np.uint64(U64)).all() and pairs[:, 1].tolist() == [j[3] for j in jobs]
        head = meta[extra["list_at"]:extra["list_at"] + LIST_HEAD].view(np.uint32).tolist()
        assert head == [0, extra["list_cap"], 0, 0] and extra["list_cap"] >= len(jobs)
        assert extra["upload_bytes"] == extra["list_at"] + LIST_HEAD
        regions += [(extra["thresh_at"], extra["thresh_bytes"]),
                    (extra["list_at"], LIST_HEAD + extra["entry_bytes"] * extra["list_cap"])]
        assert all(at % 16 == 0 for at, _ in regions) and regions == sorted(regions)
        assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))
        assert regions[-1][0] + regions[-1][1] <= meta.nbytes and meta.nbytes % 16 == 0


@pytest.mark.parametrize("win", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_one_job_stage_holds_the_single_searchs_descriptors(hc, win):
    name, mlen, policy, lo, cnt, _ = win
    m = window_msg(name, mlen)
    hc.hostcheck_set_layout_policy(policy)
    for rchunk in (0, 7):
        groups, extra, meta = stage_first(hc, [(m, lo, lo + cnt - 1, 12345)], rchunk)
        out = np.zeros((64, len(FIELDS)), dtype=np.uint64)
        size = u64()
        n = hc.hostcheck_stage(m, len(m), lo, lo + cnt - 1, rchunk, out.ctypes.data_as(pu64), 64, ctypes.byref(size),
                               None, 0)
        single = np.zeros(size.value // 8, dtype=np.uint64)
        assert hc.hostcheck_stage(m, len(m), lo, lo + cnt - 1, rchunk, out.ctypes.data_as(pu64), 64,
                                  ctypes.byref(size), single.ctypes.data, single.nbytes) == n
        sg = [dict(zip(FIELDS, (int(v) for v in row))) for row in out[:n]]
        # lane-table descriptors carry the position of their p-table in the group's room, which
        # the grouping decides: compared without it
        def strip(raw, c2):
            w = np.frombuffer(raw, dtype=np.uint32).copy()
            if c2 == 3:
                w[139] = 0
            return w.tobytes()
        theirs = sorted(strip(bytes(w.tobytes()), g["C2"]) for g in sg for w in descriptors(single.view(np.uint8), g))
        mine = sorted(strip(bytes(w.tobytes()), g["C2"]) for g in groups for w in descriptors(meta, g))
        assert mine == theirs and len(mine) > 0
        assert len(groups) >= n and sum(g["nonces"] for g in groups) == cnt
        assert extra["thresh_bytes"] == 16


# ---- 5. code generation of the MODE 5 plain kernels ----

def _tools():
    return shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))


def test_plain_first_batch_kernels_fit_8_waves_and_keep_the_loop(tmp_path):
    if not _tools():
        pytest.skip("binutils / ROCm LLVM tools not present")
    objs = {}
    for tu in ("kernels_plain_firstbatch", "kernels_plain"):
        objs[tu] = os.path.join(PKG, "build", tu + ".o")
        if not os.path.exists(objs[tu]):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{tu}.o"])
    bdir, pdir = tmp_path / "firstbatch", tmp_path / "plain"
    bdir.mkdir()
    pdir.mkdir()
    meta = kernel_metadata(objs["kernels_plain_firstbatch"], bdir)
    scans = {}
    for name, v in meta.items():
        m = re.search(r"k_scanILi(\d+)ELi0ELb0ELi5E", name)  # MODE 5
        if m:
            scans[int(m.group(1))] = v
    assert sorted(scans) == list(range(14)), scans
    for J, (vgpr, spill) in scans.items():
        assert vgpr <= 64, (J, vgpr)  # 8 waves per SIMD
    assert scans[4][1] == 0 and scans[13][1] == 0, scans
    # J = 4 and J = 13: one per-nonce loop body, no more VALU work than MODE 0's, opening at 4 mod 8
    kernel_metadata(objs["kernels_plain"], pdir)
    for J in (4, 13):
        mine = loop_bodies(bdir / "k.co", f"_ZN7gpuhash6k_scanILi{J}ELi0ELb0ELi5EE")
        plain = loop_bodies(pdir / "k.co", f"_ZN7gpuhash6k_scanILi{J}ELi0ELb0ELi0EE")
        assert len(mine) == 1 and len(plain) == 1, (J, mine, plain)
        assert mine[0][1] <= plain[0][1], (J, mine, plain)
        pins = [p for p in pinned_runs(bdir / "k.co", f"_ZN7gpuhash6k_scanILi{J}ELi0ELb0ELi5EE") if p is not None]
        assert len(pins) == 1 and pins[0] % 8 == 4, (J, pins)


# ---- 6. sanitizers ----

def test_first_batch_replay_stand_alone_under_asan_ubsan():
    """A program with its own main over hostcheck_first_below_batch (csrc/hostcheck_firstbatch_main.cpp),
    built with -fsanitize=address,undefined: 330 jobs with every kind of target under every policy,
    ranges from 0 over several digit counts, sub-batches down to one job each, three context
    entries and the top of uint64; each job checked against an ascending scan that stops at its
    first hit, and what the replay hashed against the order's property."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/hostcheck_firstbatch_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIBDIR, "hostcheck_firstbatch_asan")], env=env, capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.strip() == "ok", out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
