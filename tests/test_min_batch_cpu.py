"""CPU: gpuhash_min_batch -- many independent (message, lower, upper) searches in one call,
each answered exactly as gpuhash_min answers it.

No GPU here: the ABI's exports and argument checks, the CPU replay of the kernel's batch mode
(hostcheck_min_batch: the batch stage as fill() writes it, groups, pieces in a seeded order with
several workgroups in flight, the descriptor lookup, the job-change flush, per-job pruning words
and the result list with its bound) against the oracle, the batch stage's layout, the sub-batch
cut, the code generation of the MODE 4 plain kernels, and a stand-alone sanitizer run of the
replay.  Expected values come from oracle.hash_range + numpy argmin (tests/batch_jobs.py).
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
from test_codegen import kernel_metadata, pinned_runs
from test_collect_below_cpu import WINDOWS, window_msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
LLVM = "/opt/rocm/lib/llvm/bin"
U64 = (1 << 64) - 1
u64, u32, sz = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
pu64 = ctypes.POINTER(u64)
AUTO, UNIFORM, CLASSIC, LANETABLE, TAIL_ALWAYS = 0, 1, 2, 3, 16
FUNCS = ("gpuhash_min_batch", "gpuhash_min_batch_ex")
MAX_JOBS, MAX_SPAN = 1 << 16, 1 << 38
ORDERS = [0, 1, 12345, 987654321]  # ascending, descending, two shuffles
DESC_BYTES = 592
# 32-bit word positions in LaunchDesc (plan.h): U at 0..15, ..., R at 132, tab_off at 139, job last
DESC_R, DESC_TAB_OFF, DESC_JOB = 132, 139, 147
FIELDS = "J C2 EX ndesc d c total nonces work_at offs_at desc_at ptab_at desc_bytes ptab_bytes".split()
EXTRA = "upload_bytes thresh_at thresh_bytes list_at list_cap entry_bytes ntabs tab_words".split()
LIST_HEAD = 16


# ---- 1. exports and checks ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_min_batch(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", src), f
        assert f in exported, f  # unmangled extern "C"
        assert hasattr(lib, f)
    assert re.search(r"#define\s+GPUHASH_BATCH_MAX_JOBS\s+\(1u << 16\)", src)
    assert re.search(r"#define\s+GPUHASH_BATCH_MAX_SPAN\s+\(1ull << 38\)", src)
    import gpuhash
    assert set(FUNCS) <= set(gpuhash.EXPORTED)
    assert hasattr(gpuhash.Engine, "min_batch")
    assert (gpuhash.GPUHASH_BATCH_MAX_JOBS, gpuhash.GPUHASH_BATCH_MAX_SPAN) == (MAX_JOBS, MAX_SPAN)


def test_version_is_at_least_0_6(lib):
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 6)


def test_min_batch_argument_errors_need_no_device(lib):
    import gpuhash
    EINVAL, ETOOLONG = gpuhash.GPUHASH_EINVAL, gpuhash.GPUHASH_ETOOLONG
    ctx = ctypes.c_void_p(1)  # never dereferenced: every check below precedes any use of it
    f, fx = lib.gpuhash_min_batch, lib.gpuhash_min_batch_ex
    msgs = ctypes.create_string_buffer(b"abcdef")
    mp = ctypes.addressof(msgs)
    off = (sz * 3)(0, 3, 6)
    lo, hi = (u64 * 2)(0, 5), (u64 * 2)(9, 5)
    h, n = (u64 * 2)(7, 7), (u64 * 2)(7, 7)

    def both(want, ctx_, mp_, off_, nj, lo_, hi_, h_, n_):
        assert f(ctx_, mp_, off_, nj, lo_, hi_, h_, n_) == want
        assert fx(ctx_, mp_, off_, nj, lo_, hi_, 7, h_, n_) == want

    both(EINVAL, None, mp, off, 2, lo, hi, h, n)             # null pointers, one at a time
    both(EINVAL, ctx, None, off, 2, lo, hi, h, n)            #   (non-empty messages need msgs)
    both(EINVAL, ctx, mp, None, 2, lo, hi, h, n)
    both(EINVAL, ctx, mp, off, 2, None, hi, h, n)
    both(EINVAL, ctx, mp, off, 2, lo, None, h, n)
    both(EINVAL, ctx, mp, off, 2, lo, hi, None, n)
    both(EINVAL, ctx, mp, off, 2, lo, hi, h, None)
    both(EINVAL, ctx, mp, off, 0, lo, hi, h, n)              # njobs == 0
    big = MAX_JOBS + 1                                       # njobs > GPUHASH_BATCH_MAX_JOBS
    both(EINVAL, ctx, mp, (sz * (big + 1))(), big, (u64 * big)(), (u64 * big)(), (u64 * big)(), (u64 * big)())
    both(EINVAL, ctx, mp, (sz * 3)(0, 4, 3), 2, lo, hi, h, n)          # msg_off decreases
    both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 6), hi, h, n)           # lower[1] > upper[1]
    both(EINVAL, ctx, mp, off, 2, lo, (u64 * 2)(9, 5 + MAX_SPAN), h, n)  # a span above the maximum
    both(EINVAL, ctx, mp, off, 2, (u64 * 2)(0, 0), (u64 * 2)(9, U64), h, n)
    long_off = (sz * 3)(0, 3, 3 + gpuhash.GPUHASH_MAX_MSG + 1)         # a message over GPUHASH_MAX_MSG
    both(ETOOLONG, ctx, mp, long_off, 2, lo, hi, h, n)                 #   (its bytes are never read)
    both(EINVAL, ctx, mp, long_off, 2, (u64 * 2)(0, 6), hi, h, n)      # ... an EINVAL elsewhere comes first
    assert list(h) == [7, 7] and list(n) == [7, 7]  # nothing written


def test_binding_refuses_bad_jobs_before_calling_in():
    import gpuhash
    eng = gpuhash.Engine.__new__(gpuhash.Engine)  # no context: the checks come first
    eng._ctx = None
    for jobs in ([], [(b"x", 5, 4)], [(b"x", 0, 4), (b"y", -1, 4)], [(b"x", 0, 1 << 64)], [(b"x", 0, MAX_SPAN)],
                 [(b"x", 0)], [(bytes(gpuhash.GPUHASH_MAX_MSG + 1), 0, 1)]):
        with pytest.raises(ValueError):
            eng.min_batch(jobs)
    with pytest.raises(TypeError):
        eng.min_batch([(b"x", 0.0, 4)])
    with pytest.raises(ValueError):
        eng.min_batch([(b"x", 0, 4)], rchunk=-1)


# ---- 2. the replay against the oracle ----

@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_min_batch.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int, vp, vp, vp]
    lib.hostcheck_stage_batch.argtypes = [vp, vp, u64, vp, vp, u32, vp, ctypes.c_int, pu64, vp, vp, u64]
    lib.hostcheck_stage.argtypes = [ctypes.c_char_p, u64, u64, u64, u32, pu64, ctypes.c_int, pu64, vp, u64]
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


def replay(hc, jobs, rchunk=0, policy=AUTO, order=0, batch_bytes=0, nshards=1):
    """hostcheck_min_batch over (message, lower, upper) jobs: ([(hash, nonce)], fill) with fill =
    (largest list fill of a run, that run's bound, runs over their bound, sub-batches)."""
    msgs, off, lower, upper = batch_jobs.flat(jobs)
    h = np.full(len(jobs), 0xDEADBEEF, dtype=np.uint64)
    n = np.full(len(jobs), 0xDEADBEEF, dtype=np.uint64)
    fill = np.zeros(4, dtype=np.uint64)
    rc = hc.hostcheck_min_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data, upper.ctypes.data,
                                rchunk, policy, order, batch_bytes, nshards, h.ctypes.data, n.ctypes.data,
                                fill.ctypes.data)
    assert rc == 0
    return list(zip(h.tolist(), n.tolist())), tuple(int(v) for v in fill)


@pytest.fixture(scope="module")
def mix(oracle):
    """The job mix as (message, lower, upper) jobs, and the oracle's answers."""
    named = batch_jobs.job_mix()
    return [(m, a, b) for _, m, a, b in named], batch_jobs.expected(oracle, named)


def test_the_job_mix_is_what_the_issue_asks_for(mix):
    jobs, _ = mix
    assert 150 <= len(jobs) <= 250 and max(b - a + 1 for _, a, b in jobs) <= 5000
    assert {len(m) for m, _, _ in jobs} == {w[1] for w in WINDOWS} and len({w[1] for w in WINDOWS}) == 7
    assert (jobs[0][0] != jobs[1][0]) and any(a == b == U64 for _, a, b in jobs)
    assert sum(a == b for _, a, b in jobs) >= 24  # single-nonce jobs
    assert batch_jobs.POLICIES == [AUTO, UNIFORM, CLASSIC, LANETABLE, AUTO | TAIL_ALWAYS]


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_replay_matches_the_oracle(hc, mix, policy, rchunk):
    jobs, want = mix
    for order in ORDERS:
        got, fill = replay(hc, jobs, rchunk, policy, order)
        bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (order, bad[:3])
        assert fill[2] == 0 and 0 < fill[0] <= fill[1] and fill[3] == 1, (order, fill)


def test_replay_over_several_entries(hc, mix):
    jobs, want = mix
    for order in (0, 12345):
        got, fill = replay(hc, jobs, 0, AUTO, order, nshards=3)
        assert got == want and fill[2] == 0


# ---- 3. permutation ----

def test_permuting_the_jobs_permutes_the_results(hc, mix):
    jobs, want = mix
    perm = list(range(len(jobs)))
    random.Random("min-batch permutation").shuffle(perm)
    for order in (0, 987654321):
        got, _ = replay(hc, [jobs[i] for i in perm], 0, AUTO, order)
        assert got == [want[i] for i in perm]
    back = list(reversed(range(len(jobs))))
    got, _ = replay(hc, [jobs[i] for i in back], 7, LANETABLE, 1)
    assert got == [want[i] for i in back]


# ---- 4. the batch stage ----

def stage_batch(hc, jobs, rchunk=0):
    """(groups as dicts of FIELDS, extra as a dict of EXTRA, the metadata buffer as fill() writes it)."""
    msgs, off, lower, upper = batch_jobs.flat(jobs)
    out = np.zeros((64, len(FIELDS)), dtype=np.uint64)
    extra = np.zeros(8, dtype=np.uint64)
    size = u64()
    args = (msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data, upper.ctypes.data, rchunk,
            out.ctypes.data, 64, ctypes.byref(size), extra.ctypes.data)
    n = hc.hostcheck_stage_batch(*args, None, 0)
    assert 0 < n <= 64
    meta = np.zeros(size.value // 8, dtype=np.uint64)
    assert hc.hostcheck_stage_batch(*args, meta.ctypes.data, meta.nbytes) == n and size.value == meta.nbytes
    return ([dict(zip(FIELDS, (int(v) for v in row))) for row in out[:n]],
            dict(zip(EXTRA, (int(v) for v in extra))), meta.view(np.uint8))


def descriptors(meta, g):
    return meta[g["desc_at"]:g["desc_at"] + g["desc_bytes"]].view(np.uint32).reshape(g["ndesc"], DESC_BYTES // 4)


@pytest.mark.parametrize("win", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_one_job_batch_stages_what_a_single_search_stages(hc, win):
    name, mlen, policy, lo, cnt, _ = win
    m = window_msg(name, mlen)
    hc.hostcheck_set_layout_policy(policy)
    for rchunk in (0, 7):
        groups, extra, meta = stage_batch(hc, [(m, lo, lo + cnt - 1)], rchunk)
        out = np.zeros((64, len(FIELDS)), dtype=np.uint64)
        size = u64()
        single = np.zeros(extra["thresh_at"] // 8, dtype=np.uint64)
        n = hc.hostcheck_stage(m, len(m), lo, lo + cnt - 1, rchunk, out.ctypes.data_as(pu64), 64, ctypes.byref(size),
                               single.ctypes.data, single.nbytes)
        # the regions a single stage has: the same places, the same bytes (job index 0 included)
        assert size.value == extra["thresh_at"] == single.nbytes
        assert [dict(zip(FIELDS, (int(v) for v in row))) for row in out[:n]] == groups
        assert (meta[:extra["thresh_at"]] == single.view(np.uint8)).all()
        assert extra["thresh_bytes"] == 8 and extra["upload_bytes"] == extra["list_at"] + LIST_HEAD


def test_multi_job_stage(hc, mix):
    jobs, _ = mix
    seen_tables = 0
    for policy in batch_jobs.POLICIES:
        hc.hostcheck_set_layout_policy(policy)
        groups, extra, meta = stage_batch(hc, jobs)
        assert len({(g["J"], g["C2"], g["EX"]) for g in groups}) == len(groups)
        regions = [(0, 40 * len(groups))]
        tables = {}
        for g in groups:
            words = descriptors(meta, g)
            job = words[:, DESC_JOB].astype(np.int64)
            # grouped by job, ascending: a job's descriptors are contiguous
            assert (np.diff(job) >= 0).all() and job.max() < len(jobs)
            assert len(set(job.tolist())) > 4  # every group has many job changes
            # offs is the prefix sum of the descriptors' row-iterations
            offs = meta[g["offs_at"]:g["offs_at"] + 8 * (g["ndesc"] + 1)].view(np.uint64).tolist()
            rows = [((int(w[136]) - int(w[135])) // 256 + 1) * int(w[DESC_R]) for w in words]
            assert offs == [sum(rows[:k]) for k in range(len(rows) + 1)] and g["total"] == offs[-1]
            regions += [(g["offs_at"], 8 * (g["ndesc"] + 1)), (g["desc_at"], g["desc_bytes"]),
                        (g["ptab_at"], g["ptab_bytes"])]
            if (g["J"], g["C2"]) == (0, 1):  # K+W tables: shared exactly between equal block-B words and R
                for w in words:
                    key = (bytes(w[:16].tobytes()), int(w[DESC_R]))
                    assert tables.setdefault(key, int(w[DESC_TAB_OFF])) == int(w[DESC_TAB_OFF])
        # distinct keys have distinct, disjoint tables that tile tab_words
        spans = sorted((off, 64 * key[1]) for key, off in tables.items())
        assert len(spans) == extra["ntabs"]
        assert all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
        assert (spans[-1][0] + spans[-1][1] if spans else 0) == extra["tab_words"]
        seen_tables += len(spans)
        # the batch's regions come after the groups': per-job pruning words armed to all ones,
        # then the list (head: no entries yet, the capacity)
        regions += [(extra["thresh_at"], extra["thresh_bytes"]),
                    (extra["list_at"], LIST_HEAD + extra["entry_bytes"] * extra["list_cap"])]
        assert extra["thresh_bytes"] == 8 * len(jobs)
        assert (meta[extra["thresh_at"]:extra["thresh_at"] + extra["thresh_bytes"]] == 0xFF).all()
        head = meta[extra["list_at"]:extra["list_at"] + LIST_HEAD].view(np.uint32).tolist()
        assert head == [0, extra["list_cap"], 0, 0] and extra["list_cap"] >= len(jobs)
        assert all(at % 16 == 0 for at, _ in regions)
        assert regions == sorted(regions)
        assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))
        assert regions[-1][0] + regions[-1][1] <= meta.nbytes and meta.nbytes % 16 == 0
    assert seen_tables > 0


def test_jobs_of_one_message_share_their_tables(hc):
    """A K+W table is keyed by what it is computed from.  Two jobs of one 120-byte message in one
    digit group share one, and so does a job of ANOTHER message of that length: block B then
    holds four digits and the padding, no message byte.  A message one block longer has the same
    layout and R but another bit length in block B, and gets a table of its own."""
    m1, m2, m3 = window_msg("ktab", 120), window_msg("ktab-other", 120), window_msg("ktab-longer", 184)
    hc.hostcheck_set_layout_policy(AUTO)
    lo = 10 ** 10
    for jobs, ntabs in (([(m1, lo, lo + 999), (m1, lo + 500, lo + 2999)], 1),
                        ([(m1, lo, lo + 999), (m2, lo + 500, lo + 2999)], 1),
                        ([(m1, lo, lo + 999), (m3, lo + 500, lo + 2999)], 2)):
        groups, extra, meta = stage_batch(hc, jobs)
        assert [(g["J"], g["C2"]) for g in groups] == [(0, 1)] and extra["ntabs"] == ntabs
        offs = {int(w[DESC_JOB]): int(w[DESC_TAB_OFF]) for w in descriptors(meta, groups[0])}
        assert (offs[0] == offs[1]) == (ntabs == 1)


# ---- 5. sub-batches ----

def test_sub_batches_do_not_change_the_results(hc, mix, monkeypatch):
    jobs, want = mix
    small = 256 * 1024
    for policy, order in ((AUTO, 0), (LANETABLE, 12345)):
        got, fill = replay(hc, jobs, 0, policy, order, batch_bytes=small)
        assert got == want and fill[3] >= 3 and fill[2] == 0, fill
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", str(small))  # the override the engine reads
    got, fill = replay(hc, jobs, 7, AUTO, 1, nshards=2)
    assert got == want and fill[3] >= 3 and fill[2] == 0, fill
    monkeypatch.setenv("GPUHASH_BATCH_BYTES", "1")  # every job a sub-batch of its own
    got, fill = replay(hc, jobs[:40], 0, AUTO, 0)
    assert got == want[:40] and fill[3] == 40


# ---- 6. code generation of the MODE 4 plain kernels ----

def _tools():
    return shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))


def loop_bodies(co, kernel):
    """(instructions, VALU, SALU) of every straight-line run of >= 500 VALU instructions."""
    d = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", str(co)], text=True)
    i = d.index("<" + kernel)
    runs, cur = [], []
    for line in d[i:d.index("s_endpgm", i)].split("\n"):
        m = re.match(r"\s+([vs]_\S+|global_\S+|scratch_\S+|ds_\S+|buffer_\S+|flat_\S+)\s.*//\s*[0-9A-Fa-f]+:", line)
        if not m:
            continue
        cur.append(m.group(1))
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            runs.append(cur)
            cur = []
    return [(len(r), sum(op.startswith("v_") for op in r), sum(op.startswith("s_") for op in r))
            for r in runs if sum(op.startswith("v_") for op in r) >= 500]


def test_plain_batch_kernels_fit_8_waves_and_keep_the_loop(tmp_path):
    if not _tools():
        pytest.skip("binutils / ROCm LLVM tools not present")
    objs = {}
    for tu in ("kernels_plain_batch", "kernels_plain"):
        objs[tu] = os.path.join(PKG, "build", tu + ".o")
        if not os.path.exists(objs[tu]):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{tu}.o"])
    bdir, pdir = tmp_path / "batch", tmp_path / "plain"
    bdir.mkdir()
    pdir.mkdir()
    meta = kernel_metadata(objs["kernels_plain_batch"], bdir)
    scans = {}
    for name, v in meta.items():
        m = re.search(r"k_scanILi(\d+)ELi0ELb0ELi4E", name)  # MODE 4
        if m:
            scans[int(m.group(1))] = v
    assert sorted(scans) == list(range(14)), scans
    for J, (vgpr, spill) in scans.items():
        assert vgpr <= 64, (J, vgpr)  # 8 waves per SIMD
    assert scans[4][1] == 0 and scans[5][1] == 0, scans
    # J = 4: one per-nonce loop body, no more VALU work than MODE 0's, opening at 4 mod 8
    kernel_metadata(objs["kernels_plain"], pdir)
    batch = loop_bodies(bdir / "k.co", "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi4EE")
    plain = loop_bodies(pdir / "k.co", "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi0EE")
    assert len(batch) == 1 and len(plain) == 1, (batch, plain)
    assert batch[0][1] <= plain[0][1], (batch, plain)
    pins = [p for p in pinned_runs(bdir / "k.co", "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi4EE") if p is not None]
    assert len(pins) == 1 and pins[0] % 8 == 4, pins


# ---- 7. sanitizers ----

def test_batch_replay_stand_alone_under_asan_ubsan():
    """A program with its own main over hostcheck_min_batch (csrc/hostcheck_batch_main.cpp), built
    with -fsanitize=address,undefined: 330 jobs under every policy, sub-batches down to one job
    each, three context entries and the top of uint64, each job checked against an ascending scan."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/hostcheck_batch_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIBDIR, "hostcheck_batch_asan")], env=env, capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.strip() == "ok", out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
