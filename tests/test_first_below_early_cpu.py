"""CPU: gpuhash_first_below_batch_early -- gpuhash_first_below_batch's answers, with the front of
every job hashed packed in ascending rounds of doubling pieces.

No GPU here: the ABI's export and argument checks, the rule for a job's packed front against the
header's text, the CPU replay of the whole call (hostcheck_first_below_batch_early: the rule, the
rounds and their sub-batches, k_pack_first over every round's tiles in seeded orders with stale
bound reads, the bounded store, the remainder through the first-hit batch replay) against the
oracle, the work bound 2x + c_0, the list capacity, the new kernel's code generation, and a
stand-alone sanitizer run of the replay.  Expected values come from oracle.hash_range + numpy.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import batch_jobs
import first_batch_jobs
import packed_jobs
from first_batch_jobs import first_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
GOLDEN_MANIFEST = os.path.join(ROOT, "tests", "golden", "kernel_manifest_early.txt")
U64 = (1 << 64) - 1
u64, u32, sz = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
AUTO = 0
FUNC = "gpuhash_first_below_batch_early"
MAX_JOBS, MAX_SPAN = 1 << 16, 1 << 38
ORDERS = [0, 1, 12345, 987654321]  # ascending, descending, two shuffles
PREFIXES = [0, 1, 64, 1000, 1 << 20]
MARK = 0xDEADBEEF
ROUND_ITEMS = 1 << 20
# the digit-boundary jobs: a boundary five to a hundred nonces in (10^19 among them), the top of uint64
BOUNDARY_LOWERS = [95, 9990, 99999990, 10 ** 19 - 100, (1 << 64) - 5001]
BOUNDARY_FROM = 3000


def header_max_prefix():
    m = re.search(r"#define\s+GPUHASH_EARLY_MAX_PREFIX\s+\(1u << (\d+)\)", open(HEADER).read())
    assert m
    return 1 << int(m.group(1))


def limit_of(lo, hi, target, prefix):
    """The header's rule, in exact integers."""
    span = hi - lo + 1
    if prefix:
        return min(span, prefix)
    e = -((-(1 << 64)) // (target + 1))  # ceil(2^64 / (target + 1))
    return min(span, 4 * e) if 4 * e <= header_max_prefix() else 0


def first_chunk(fronts):
    want = ROUND_ITEMS // fronts if fronts else ROUND_ITEMS
    c = 1
    while c < want:
        c *= 2
    return min(max(c, 64), ROUND_ITEMS)


# ---- 1. exports, checks, the rule ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_it(lib):
    import gpuhash
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    proto = re.search(r"\bint\s+" + FUNC + r"\s*\(([^)]*)\)", src)
    assert proto and FUNC in exported and hasattr(lib, FUNC)
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    assert args == ["gpuhash_ctx *ctx", "const uint8_t *msgs", "const size_t *msg_off", "size_t njobs",
                    "const uint64_t *lower", "const uint64_t *upper", "const uint64_t *target", "uint64_t prefix",
                    "uint32_t rchunk", "uint64_t *out_hashes", "uint64_t *out_nonces", "int *out_found"]
    assert len(lib.gpuhash_first_below_batch_early.argtypes) == len(args)
    assert FUNC in gpuhash.EXPORTED and FUNC + "_ex" not in gpuhash.EXPORTED  # one function, no twin
    assert hasattr(gpuhash.Engine, "first_below_batch_early")
    assert gpuhash.EARLY_MAX_PREFIX == header_max_prefix() <= 16 * gpuhash.PACKED_MAX_SPAN
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 9)


def test_argument_errors_need_no_device(lib):
    import gpuhash
    EINVAL, ETOOLONG = gpuhash.GPUHASH_EINVAL, gpuhash.GPUHASH_ETOOLONG
    f = lib.gpuhash_first_below_batch_early
    msgs = ctypes.create_string_buffer(b"abcdef")
    mp = ctypes.addressof(msgs)
    off = (sz * 3)(0, 3, 6)
    lo, hi, tg = (u64 * 2)(0, 5), (u64 * 2)(9, 5), (u64 * 2)(U64, U64)
    h, n, fd = (u64 * 2)(7, 7), (u64 * 2)(7, 7), (ctypes.c_int * 2)(7, 7)
    garbage = ctypes.create_string_buffer(b"\xA5" * 64, 64)  # not a context: never read as one
    assert f(None, mp, off, 2, lo, hi, tg, 0, 0, h, n, fd) == EINVAL
    for ctx in (ctypes.c_void_p(1), ctypes.c_void_p(ctypes.addressof(garbage))):
        for prefix, rchunk in ((0, 0), (1000, 7)):
            def call(want, mp_=mp, off_=off, nj=2, lo_=lo, hi_=hi, tg_=tg, h_=h, n_=n, fd_=fd, prefix_=prefix):
                assert f(ctx, mp_, off_, nj, lo_, hi_, tg_, prefix_, rchunk, h_, n_, fd_) == want
            call(EINVAL, mp_=None)
            call(EINVAL, off_=None)
            call(EINVAL, lo_=None)
            call(EINVAL, hi_=None)
            call(EINVAL, tg_=None)
            call(EINVAL, h_=None)
            call(EINVAL, n_=None)
            call(EINVAL, fd_=None)
            call(EINVAL, nj=0)
            big = MAX_JOBS + 1
            call(EINVAL, off_=(sz * (big + 1))(), nj=big, lo_=(u64 * big)(), hi_=(u64 * big)(), tg_=(u64 * big)(),
                 h_=(u64 * big)(), n_=(u64 * big)(), fd_=(ctypes.c_int * big)())
            call(EINVAL, off_=(sz * 3)(0, 4, 3))                      # msg_off decreases
            call(EINVAL, lo_=(u64 * 2)(0, 6))                         # lower[1] > upper[1]
            call(EINVAL, hi_=(u64 * 2)(9, 5 + MAX_SPAN))              # a span above the maximum
            call(EINVAL, prefix_=MAX_SPAN + 1)                        # the new one
            call(EINVAL, prefix_=U64)
            long_off = (sz * 3)(0, 3, 3 + gpuhash.GPUHASH_MAX_MSG + 1)
            call(ETOOLONG, off_=long_off)
            call(EINVAL, off_=long_off, lo_=(u64 * 2)(0, 6))          # an EINVAL elsewhere comes first
    assert list(h) == [7, 7] and list(n) == [7, 7] and list(fd) == [7, 7]  # nothing written
    assert garbage.raw == b"\xA5" * 64


def test_binding_refuses_bad_jobs_before_calling_in():
    import gpuhash
    eng = gpuhash.Engine.__new__(gpuhash.Engine)  # no context: the checks come first
    eng._ctx = None
    for jobs in ([], [(b"x", 5, 4, 0)], [(b"x", 0, MAX_SPAN, 0)], [(b"x", 0, 4)], [(b"x", 0, 4, 1 << 64)]):
        with pytest.raises(ValueError):
            eng.first_below_batch_early(jobs)
    for prefix in (-1, MAX_SPAN + 1, 0.5, True):
        with pytest.raises(ValueError):
            eng.first_below_batch_early([(b"x", 0, 4, 0)], prefix=prefix)
    with pytest.raises(ValueError):
        eng.first_below_batch_early([(b"x", 0, 4, 0)], rchunk=-1)


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.hostcheck_first_below_batch_early.argtypes = [vp, vp, u64, vp, vp, vp, u64, u32, ctypes.c_int, u64, u64,
                                                      ctypes.c_int, vp, vp, vp, vp, vp]
    lib.hostcheck_early_limit.argtypes = [u64, u64, u64, u64]
    lib.hostcheck_early_limit.restype = u64
    lib.hostcheck_early_first_chunk.argtypes = [u64]
    lib.hostcheck_early_first_chunk.restype = u64
    return lib


def test_the_rule_is_the_headers(hc):
    """include/gpuhash.h states the rule once; csrc/stage.h (early_limit) implements it."""
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+GPUHASH_EARLY_MAX_PREFIX", text, flags=re.S)
    assert m
    rule = " ".join(m.group(1).replace("*", " ").split())
    for piece in ("E_k = ceil(2^64 / (target[k] + 1))", "4 E_k <= GPUHASH_EARLY_MAX_PREFIX -> limit_k = min(span_k, 4 E_k)",
                  "otherwise -> limit_k = 0", "limit_k = min(span_k, prefix)", "clamped to [64, 2^20]",
                  "c_(r+1) = min(2 c_r, 2^20)", "at most 2x + c_0 packed nonces"):
        assert piece in rule, piece
    cap = header_max_prefix()
    edge = (1 << 66) // cap  # 4 E = cap exactly where target + 1 = 2^66 / cap
    targets = [0, 1, (1 << 40) - 1, (1 << 44) - 1, (1 << 48) - 1, (1 << 52) - 1, edge - 2, edge - 1, edge, 3 * edge // 2,
               1 << 63, U64 - 1, U64]
    spans = [(0, (1 << 32) - 1), (95, 5094), (U64 - 5000, U64), (7, 7), (0, MAX_SPAN - 1)]
    seen = set()
    for t in targets:
        for lo, hi in spans:
            for prefix in (0, 1, 1000, 1 << 20, MAX_SPAN):
                want = limit_of(lo, hi, t, prefix)
                assert hc.hostcheck_early_limit(lo, hi, t, prefix) == want, (t, lo, hi, prefix)
                seen.add(0 if not want else 1 if want == hi - lo + 1 else 2)
    assert seen == {0, 1, 2}  # no front, the whole span, a front of 4 E
    assert limit_of(0, U64 >> 30, 0, 0) == 0 and limit_of(0, 99, U64, 0) == 4  # target 0: scan only
    assert limit_of(0, (1 << 32) - 1, edge - 1, 0) == cap and limit_of(0, (1 << 32) - 1, edge - 2, 0) == 0
    for fronts in (1, 2, 3, 5, 255, 256, 257, 1512, 16384, 16385, 65536):
        assert hc.hostcheck_early_first_chunk(fronts) == first_chunk(fronts), fronts


# ---- 2. the replay against the oracle ----

def replay(hc, jobs, prefix=0, rchunk=0, policy=AUTO, order=0, batch_bytes=0, nshards=1):
    """([(hash, nonce) or None], packed nonces per job, fill): fill = (largest list fill of a round's
    stage, its capacity, round stages over their capacity, round stages, remainder stages over their
    bound, c_0).  A job that is not found must leave its outputs untouched."""
    msgs, off, lower, upper, target = first_batch_jobs.flat(jobs)
    h = np.full(len(jobs), MARK, dtype=np.uint64)
    n = np.full(len(jobs), MARK, dtype=np.uint64)
    found = np.full(len(jobs), -1, dtype=np.int32)
    packed = np.zeros(len(jobs), dtype=np.uint64)
    fill = np.zeros(6, dtype=np.uint64)
    rc = hc.hostcheck_first_below_batch_early(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data,
                                              upper.ctypes.data, target.ctypes.data, prefix, rchunk, policy, order,
                                              batch_bytes, nshards, h.ctypes.data, n.ctypes.data, found.ctypes.data,
                                              packed.ctypes.data, fill.ctypes.data)
    assert rc == 0
    got = []
    for k in range(len(jobs)):
        if found[k]:
            got.append((int(h[k]), int(n[k])))
        else:
            assert (int(h[k]), int(n[k]), int(found[k])) == (MARK, MARK, 0)
            got.append(None)
    return got, [int(v) for v in packed], tuple(int(v) for v in fill)


def check(jobs, want, got, packed, fill, prefix):
    bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    limits = [limit_of(a, b, t, prefix) for _, a, b, t in jobs]
    c0 = first_chunk(sum(1 for l in limits if l))
    assert fill[5] == c0
    for (m, a, b, t), w, p, limit in zip(jobs, want, packed, limits):
        assert p <= limit
        if w is None or w[1] - a >= limit:
            assert p == limit, (a, b, t, p, limit)  # the whole front, then the remainder
        else:
            assert p <= 2 * (w[1] - a) + c0, (a, b, t, w, p, c0)  # the work bound
    assert fill[2] == 0 and fill[4] == 0 and fill[0] <= fill[1], fill
    assert first_batch_jobs.examined(jobs, got) == first_batch_jobs.examined(jobs, want)


@pytest.fixture(scope="module")
def boundary(oracle):
    """Five jobs of 5001 nonces that cross a digit boundary early; the target is the least hash from
    offset 3000 on, so the answer lies at or after it."""
    jobs, want = [], []
    for i, lo in enumerate(BOUNDARY_LOWERS):
        m = b"early-%d" % i + b"z" * (11 * i)
        hi = min(lo + 5000, U64)
        h = oracle.hash_range(m, lo, hi - lo + 1)
        t = int(h[BOUNDARY_FROM:].min())
        jobs.append((m, lo, hi, t))
        want.append(first_index(h, lo, t))
    assert any(w[1] - j[1] >= BOUNDARY_FROM for j, w in zip(jobs, want))
    return jobs, want


@pytest.fixture(scope="module")
def classes(oracle, boundary):
    """packed_jobs.matrix() with first_batch_jobs' five kinds of target cycled over it, and the
    boundary jobs at its end: beside more than a thousand jobs c_0 is 1024 or 2048, so their answers
    fall in the second or third round."""
    jobs3 = packed_jobs.matrix()
    hs = packed_jobs.hashes(oracle, jobs3)
    jobs, want = [], []
    for k, ((m, a, b), h) in enumerate(zip(jobs3, hs)):
        t = first_batch_jobs.target_of(h, k % first_batch_jobs.KINDS)
        jobs.append((m, a, b, t))
        want.append(first_index(h, a, t))
    assert any(w and w[1] == U64 for w in want) and max(len(j[0]) for j in jobs) == 1 << 20
    return jobs + boundary[0], want + boundary[1]


@pytest.fixture(scope="module")
def mix(oracle):
    return first_batch_jobs.jobs_and_answers(oracle)


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("prefix", PREFIXES)
def test_replay_of_the_class_matrix(hc, classes, prefix, rchunk):
    jobs, want = classes
    for order in ORDERS:
        got, packed, fill = replay(hc, jobs, prefix, rchunk, AUTO, order)
        check(jobs, want, got, packed, fill, prefix)
        if prefix > 2048:  # the boundary jobs' fronts took more than one round
            assert fill[5] <= 2048 and fill[3] >= 2, fill


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("prefix", PREFIXES)
def test_replay_of_the_mix(hc, mix, prefix, rchunk):
    jobs, want = mix
    for i, order in enumerate(ORDERS):
        policy = batch_jobs.POLICIES[(i + rchunk) % len(batch_jobs.POLICIES)]
        got, packed, fill = replay(hc, jobs, prefix, rchunk, policy, order)
        check(jobs, want, got, packed, fill, prefix)


def test_boundary_answers_fall_in_a_later_round(hc, classes, boundary):
    jobs, want = classes
    got, packed, fill = replay(hc, jobs, 1 << 20, 0, AUTO, 12345)
    c0 = fill[5]
    assert c0 == 1024
    later = 0
    for (m, a, b, t), w, p in zip(jobs[-5:], want[-5:], packed[-5:]):
        x = w[1] - a
        assert p <= 2 * x + c0, (a, x, p)
        later += x >= c0 and p > c0  # (an earlier nonce may beat the least hash from offset 3000 on)
        assert len(str(a)) < len(str(w[1])) or a > U64 - 6000  # the boundary lies before the answer
    assert later >= 3, later  # not in the first round


def test_entries_and_sub_batches_do_not_change_the_results(hc, mix, classes):
    jobs, want = mix
    for prefix, order, nshards, small in ((0, 12345, 3, 0), (1000, 1, 2, 16 * 1024), (1 << 20, 987654321, 3, 16 * 1024),
                                          (64, 0, 1, 1)):
        got, packed, fill = replay(hc, jobs, prefix, 0, AUTO, order, batch_bytes=small, nshards=nshards)
        check(jobs, want, got, packed, fill, prefix)
        if small:
            assert fill[3] >= 3, fill
    jobs, want = classes
    got, packed, fill = replay(hc, jobs, 1 << 20, 7, AUTO, 12345, batch_bytes=256 * 1024, nshards=3)
    check(jobs, want, got, packed, fill, 1 << 20)
    assert fill[3] >= 4, fill


# ---- 3. the kernel's code generation ----

def test_the_early_kernel_is_the_recorded_one():
    """build/pack_first.o against tests/golden/kernel_manifest_early.txt: no scratch, no VGPR spill
    (metadata only).  After an intended change or a compiler update:
    python tools/kernel_manifest.py bitcoin-miner_amd/build/pack_first.o"""
    if not (shutil.which("objcopy") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")):
        pytest.skip("binutils / ROCm LLVM tools not present")
    obj = os.path.join(PKG, "build", "pack_first.o")
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-s", "-C", PKG, "build/pack_first.o"])
    built = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_manifest.py"), obj], text=True)
    lines = built.splitlines()
    assert lines == open(GOLDEN_MANIFEST).read().splitlines() and len(lines) == 1 and "k_pack_first" in lines[0]
    f = dict(kv.split("=") for kv in lines[0].split(" ")[2:])
    assert f["private_segment_fixed_size"] == "0" and f["vgpr_spill_count"] == "0", lines[0]
    assert f["group_segment_fixed_size"] == "16" and int(f["vgpr_count"]) <= 128, lines[0]
    import glob
    assert obj not in glob.glob(os.path.join(PKG, "build", "kernels*.o"))


# ---- 4. sanitizers ----

def test_early_replay_stand_alone_under_asan_ubsan():
    """A program with its own main over hostcheck_first_below_batch_early
    (csrc/hostcheck_early_main.cpp), built with -fsanitize=address,undefined: digit boundaries
    inside a chunk and between rounds, the top of uint64, a prefix of 1 and of the span and more,
    sub-batches and three entries; each job checked against an ascending scan."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/hostcheck_early_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIBDIR, "hostcheck_early_asan")], env=env, capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.strip() == "ok", out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
