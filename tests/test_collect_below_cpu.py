"""CPU: gpuhash_collect_below -- every nonce of a range whose hash is at or below a target:
the exact count, and the lowest `cap` of them.

No GPU here: the ABI's argument checks, the CPU replay of the kernel's collecting mode
(hostcheck_collect_below: the same plan, pieces and masks, a device list of `buffer_entries`
entries that drops appends past its end, the append order chosen by a seed, and the engine's
own collector, csrc/collect.h) against the oracle, the collector's corner cases, and the code
generation of the MODE 3 plain kernels.  Expected values come from oracle.hash_range + numpy.
"""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
LLVM = "/opt/rocm/lib/llvm/bin"
U64 = (1 << 64) - 1
u64, u32 = ctypes.c_uint64, ctypes.c_uint32
AUTO, UNIFORM, CLASSIC, LANETABLE, TAIL_ALWAYS = 0, 1, 2, 3, 16
COLLECT_MAX = 1 << 20
FUNCS = ("gpuhash_collect_below", "gpuhash_collect_below_ex")


# ---- 1. header and library ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_collect_below(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", src), f
        assert f in exported, f  # unmangled extern "C"
        assert hasattr(lib, f)
    assert re.search(r"#define\s+GPUHASH_COLLECT_MAX\s+\(1u << 20\)", src)
    import gpuhash
    assert set(FUNCS) <= set(gpuhash.EXPORTED)
    assert hasattr(gpuhash.Engine, "collect_below") and hasattr(gpuhash.Engine, "count_below")
    assert gpuhash.GPUHASH_COLLECT_MAX == COLLECT_MAX


def test_version_is_at_least_0_5(lib):
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 5)


# ---- 2. argument errors ----

def test_collect_below_argument_errors_need_no_device(lib):
    import gpuhash
    EINVAL = gpuhash.GPUHASH_EINVAL
    n, h, t = (u64 * 4)(), (u64 * 4)(), u64()
    bt = ctypes.byref(t)
    ctx = ctypes.c_void_p(1)  # never dereferenced: every check below precedes any use of it
    f, fx = lib.gpuhash_collect_below, lib.gpuhash_collect_below_ex
    assert f(None, b"x", 1, 0, 1, 5, n, h, 4, bt) == EINVAL
    assert fx(None, b"x", 1, 0, 1, 5, 0, n, h, 4, bt) == EINVAL
    assert f(None, b"x", 1, 0, 1, 5, None, None, 0, bt) == EINVAL
    assert f(ctx, b"x", 1, 0, 1, 5, n, h, 4, None) == EINVAL
    assert f(ctx, b"x", 1, 0, 1, 5, None, None, 0, None) == EINVAL
    assert f(ctx, b"x", 1, 0, 1, 5, None, h, 4, bt) == EINVAL
    assert f(ctx, b"x", 1, 0, 1, 5, n, None, 4, bt) == EINVAL
    assert fx(ctx, b"x", 1, 0, 1, 5, 7, None, None, 1, bt) == EINVAL
    assert f(ctx, b"x", 1, 2, 1, 5, n, h, 4, bt) == EINVAL
    assert fx(ctx, b"x", 1, 2, 1, 5, 7, n, h, 4, bt) == EINVAL
    assert f(ctx, b"x", 1, 2, 1, 5, None, None, 0, bt) == EINVAL  # lower > upper as a pure count
    big_n, big_h = (u64 * (COLLECT_MAX + 1))(), (u64 * (COLLECT_MAX + 1))()
    assert f(ctx, b"x", 1, 0, 1, 5, big_n, big_h, COLLECT_MAX + 1, bt) == EINVAL
    assert fx(ctx, b"x", 1, 0, 1, 5, 0, big_n, big_h, COLLECT_MAX + 1, bt) == EINVAL
    big = bytes(gpuhash.GPUHASH_MAX_MSG + 1)
    assert f(ctx, big, len(big), 0, 1, 5, n, h, 4, bt) == gpuhash.GPUHASH_ETOOLONG
    assert fx(ctx, big, len(big), 0, 1, 5, 0, n, h, 4, bt) == gpuhash.GPUHASH_ETOOLONG
    assert f(ctx, big, len(big), 0, 1, 5, None, None, 0, bt) == gpuhash.GPUHASH_ETOOLONG
    # cap = 0 with null arrays is a valid call, which a dummy context cannot make: the GPU
    # suite's count_below makes it (tests/test_gpu_collect_below.py)
    assert t.value == 0 and list(n) == [0] * 4 and list(h) == [0] * 4  # nothing written


def test_binding_refuses_bad_target_and_cap_before_calling_in():
    import gpuhash
    eng = gpuhash.Engine.__new__(gpuhash.Engine)  # no context: the checks come first
    eng._ctx = None
    for kw in (dict(target=1 << 64), dict(target=-1), dict(target=5, cap=COLLECT_MAX + 1), dict(target=5, cap=-1)):
        with pytest.raises(ValueError):
            eng.collect_below(b"x", 0, 4, **kw)
    with pytest.raises(ValueError):
        eng.count_below(b"x", 0, 4, 1 << 64)


# ---- 3. the replay against the oracle ----

class Info(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int) for n in "J C2 EX d q s".split()]
                + [(n, u64) for n in "lo hi base".split()]
                + [(n, u32) for n in "nblocks R rchunk nrchunks p_first p_last r_first r_last".split()]
                + [(n, u32) for n in "stride tail".split()])


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    cp, pu64 = ctypes.c_char_p, ctypes.POINTER(u64)
    lib.gpuhash_plan_all.argtypes = [cp, u64, u64, u64, u32, ctypes.POINTER(Info), ctypes.c_int]
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_collect_below.argtypes = [cp, u64, u64, u64, u32, u64, ctypes.c_int, u64, u64, u64, u64,
                                            ctypes.c_int, pu64, pu64, pu64, pu64]
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


# The window family of test_first_below_cpu.py, restated: (name, message length, layout
# policy, lower, count, the (C2, J == 0, EX) a launch must have).  Every layout family, digit
# boundaries where the kernel variant changes, tail-digit launches, and the top of uint64.
WINDOWS = [
    ("plain", 8, AUTO, 10 ** 7 - 2100, 4500, (0, False, 0)),             # J = 3 -> 4
    ("plain-j0", 63, AUTO, 10 ** 4 - 2000, 4000, (0, True, 0)),          # J = 0 -> 1
    ("ktab", 120, AUTO, 10 ** 11 - 1500, 4000, (1, True, 0)),            # C2 = 1, J = 0 -> J = 1
    ("classic", 58, CLASSIC, 10 ** 9 - 2500, 5000, (1, False, 0)),       # C2 = 1, J = 1
    ("two-word", 58, UNIFORM, 10 ** 9 - 2500, 5000, (2, False, 0)),      # C2 = 2
    ("lane-table", 61, LANETABLE, 10 ** 6 - 2000, 4000, (3, False, 0)),  # K+W table -> C2 = 3
    ("lane-table-first", 61, LANETABLE, 10 ** 10 - 2000, 4000, (3, False, 0)),  # C2 = 3 -> J = 2
    ("extra-block", 42, AUTO, 10 ** 13 - 1800, 4000, (0, False, 1)),     # EX, J = 13 -> 14
    ("tail-digit", 8, AUTO | TAIL_ALWAYS, 10 ** 11 - 1700, 4200, (0, False, 0)),
    ("top-tail", 8, AUTO | TAIL_ALWAYS, U64 - 3999, 4000, (0, False, 0)),
    ("top", 8, AUTO, U64 - 3999, 4000, (0, False, 0)),
    ("top-two-blocks", 50, AUTO, U64 - 2999, 3000, None),
]
ORDERS = [0, 1, 12345, 987654321]  # ascending, descending, two shuffles
BUFFERS = [8, 64, COLLECT_MAX]
CAPS = [0, 5, COLLECT_MAX]
SENTINEL = 0xDEADBEEFDEADBEEF


def window_msg(name, mlen):
    rng = random.Random(f"first-below {name} {mlen}")
    return bytes(rng.randrange(256) for _ in range(mlen))


_hashes = {}


def window_hashes(oracle, name, m, lo, cnt):
    if name not in _hashes:  # one oracle run per window, shared and read-only
        h = oracle.hash_range(m, lo, cnt)
        h.setflags(write=False)
        _hashes[name] = h
    return _hashes[name]


def five_targets(h):
    """The window's minimum hash minus 1 (nothing qualifies), the minimum (one hit), about the
    1/1000 and the 1/64 quantiles, and 2^64-1 (every nonce)."""
    s = np.sort(h)
    return [int(s[0]) - 1, int(s[0]), int(s[max(len(s) // 1000, 1)]), int(s[len(s) // 64]), U64]


def expected(h, lo, target, cap):
    """(total, the lowest min(cap, total) hits as (nonce, hash), ascending)."""
    idx = np.nonzero(h <= np.uint64(target))[0]
    return int(idx.size), [(lo + int(i), int(h[i])) for i in idx[:cap]]


def plan(hc, m, lo, hi, rchunk):
    arr = (Info * 512)()
    n = hc.gpuhash_plan_all(m, len(m), lo, hi, rchunk, arr, 512)
    assert 0 < n <= 512
    return list(arr[:n])


class Replay:
    """hostcheck_collect_below with output arrays that are allocated once: the entries a call
    may write, and the one after them, are set to a sentinel before it."""

    def __init__(self, hc):
        self.hc = hc
        self.nonces = np.full(COLLECT_MAX, SENTINEL, dtype=np.uint64)
        self.hashes = np.full(COLLECT_MAX, SENTINEL, dtype=np.uint64)

    def __call__(self, m, lo, hi, rchunk, target, policy, order, buffer, cap, want_k, slice_nonces=0, nshards=1):
        pu64 = ctypes.POINTER(u64)
        k = min(want_k + 1, cap)
        self.nonces[:k] = SENTINEL
        self.hashes[:k] = SENTINEL
        total, runs = u64(SENTINEL), u64()
        pn = self.nonces.ctypes.data_as(pu64) if cap else None
        ph = self.hashes.ctypes.data_as(pu64) if cap else None
        rc = self.hc.hostcheck_collect_below(m, len(m), lo, hi, rchunk, target, policy, order, buffer, cap,
                                             slice_nonces, nshards, pn, ph, ctypes.byref(total), ctypes.byref(runs))
        assert rc == 0
        got = list(zip(self.nonces[:want_k].tolist(), self.hashes[:want_k].tolist()))
        if want_k < cap:  # entries from min(cap, total) on are untouched
            assert self.nonces[want_k] == SENTINEL and self.hashes[want_k] == SENTINEL
        return total.value, got, runs.value


@pytest.fixture(scope="module")
def replay(hc):
    return Replay(hc)


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("win", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_replay_is_exact_in_every_order(hc, replay, oracle, win, rchunk):
    name, mlen, policy, lo, cnt, want_variant = win
    m = window_msg(name, mlen)
    hi = lo + cnt - 1
    h = window_hashes(oracle, name, m, lo, cnt)
    hc.hostcheck_set_layout_policy(policy)
    launches = plan(hc, m, lo, hi, rchunk)
    if want_variant:
        assert any((l.C2, l.J == 0, l.EX) == want_variant for l in launches), [(l.J, l.C2, l.EX) for l in launches]
    if policy & TAIL_ALWAYS:
        assert any(l.stride == 10 for l in launches)
    for ti, target in enumerate(five_targets(h)):
        if ti in (0, 1, 4):
            assert expected(h, lo, target, 0)[0] == {0: 0, 1: 1, 4: cnt}[ti]
        for cap in CAPS:
            total, want = expected(h, lo, target, cap)
            for buffer in BUFFERS:
                for order in ORDERS:
                    got_total, got, runs = replay(m, lo, hi, rchunk, target, policy, order, buffer, cap, len(want))
                    assert got_total == total, (name, rchunk, ti, cap, buffer, order)
                    assert got == want, (name, rchunk, ti, cap, buffer, order)
                    # re-runs happen exactly when a list is wanted and the window overflows it
                    assert (runs > 1) == (cap > 0 and total > buffer), (name, ti, cap, buffer, runs)
    # every nonce a hit and a list of ONE entry: the split-and-re-run path goes down to single
    # nonces (a list of 8, above, stops at runs of 8)
    total, want = expected(h, lo, U64, COLLECT_MAX)
    got_total, got, runs = replay(m, lo, hi, rchunk, U64, policy, 12345, 1, COLLECT_MAX, len(want))
    assert (got_total, got) == (cnt, want) and runs >= cnt


def test_every_layout_family_is_replayed(hc):
    """The windows above reach C2 = 0, 1 (J = 0 and J = 1), 2, 3, an extra-block kernel and
    the tail-digit launches."""
    seen = set()
    tails = False
    for name, mlen, policy, lo, cnt, _ in WINDOWS:
        hc.hostcheck_set_layout_policy(policy)
        for l in plan(hc, window_msg(name, mlen), lo, lo + cnt - 1, 0):
            seen.add((l.C2, min(l.J, 2), l.EX))
            tails |= l.stride == 10
    assert {(0, 2, 0), (0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)} <= seen, seen
    assert any(ex for _, _, ex in seen) and tails


def test_bradfitz_known_totals(replay, oracle):
    """Checked on the CPU oracle: total 1 on [0, 9999] at the range's minimum hash, total 2 at
    target 2^52 (nonces 5103 and 9898)."""
    h = oracle.hash_range(b"bradfitz", 0, 10000)
    assert expected(h, 0, 1419516646206828, 9) == (1, [(9898, 1419516646206828)])
    assert [n for n, _ in expected(h, 0, 1 << 52, 9)[1]] == [5103, 9898]
    for order in ORDERS:
        assert replay(b"bradfitz", 0, 9999, 0, 1419516646206828, AUTO, order, 8, 9, 1)[:2] == \
            (1, [(9898, 1419516646206828)])
        total, got, _ = replay(b"bradfitz", 0, 9999, 0, 1 << 52, AUTO, order, 1, 9, 2)
        assert total == 2 and [n for n, _ in got] == [5103, 9898]


# ---- 4. the collector's corner cases, through the replay ----

@pytest.mark.parametrize("buffer", [1, 64, COLLECT_MAX])
def test_top_of_u64_every_nonce(replay, oracle, buffer):
    """[2^64-5000, 2^64-1] at target 2^64-1: total 5000 and the last hit is nonce 2^64-1, a
    legal hit; the halving of an overflowed sub-range does not wrap at the top."""
    lo = U64 - 4999
    h = oracle.hash_range(b"bradfitz", lo, 5000)
    total, want = expected(h, lo, U64, COLLECT_MAX)
    assert total == 5000 and want[-1][0] == U64
    for order in (0, 987654321):
        assert replay(b"bradfitz", lo, U64, 0, U64, AUTO, order, buffer, COLLECT_MAX, 5000)[:2] == (5000, want)
        assert replay(b"bradfitz", lo, U64, 0, U64, AUTO, order, buffer, 0, 0)[:2] == (5000, [])
    # the single nonce 2^64-1
    assert replay(b"bradfitz", U64, U64, 0, U64, AUTO, 0, buffer, 3, 1)[:2] == (1, [(U64, int(h[-1]))])


@pytest.mark.parametrize("nshards", [1, 2])
def test_full_output_stops_lists_and_reruns(replay, oracle, nshards):
    """cap is reached inside the first of five slices; every later sub-range overflows the
    list too, and is counted exactly without a list and without a re-run.  Every nonce is a
    hit, slices of 1000 nonces per shard, a list of 64: the first sub-range is halved until its
    lowest part fits, and each later sub-range runs once."""
    lo, cnt, per = 3_000_000, 5000 * nshards, 1000
    h = oracle.hash_range(b"bradfitz", lo, cnt)
    total, want = expected(h, lo, U64, 5)
    halvings, n = 0, per  # the first shard of the first slice holds `per` nonces when nshards = 1
    if nshards == 1:
        while n > 64:
            n = (n - 1) // 2 + 1
            halvings += 1
        assert halvings == 4
    for order in ORDERS:
        got_total, got, runs = replay(b"bradfitz", lo, lo + cnt - 1, 0, U64, AUTO, order, 64, 5, 5,
                                      slice_nonces=per, nshards=nshards)
        assert (got_total, got) == (cnt, want)
        if nshards == 1:
            assert runs == 5 + halvings, runs
        else:  # 10 original sub-ranges; only the first is halved, at most log2 of its size times
            assert 10 < runs <= 10 + 11, runs
    # a sparse target over the same slices: the list is ascending across slice and shard borders
    target = int(np.sort(h)[cnt // 64])
    total, want = expected(h, lo, target, COLLECT_MAX)
    assert total > 64
    for buffer in (8, COLLECT_MAX):
        assert replay(b"bradfitz", lo, lo + cnt - 1, 7, target, AUTO, 12345, buffer, COLLECT_MAX, total,
                      slice_nonces=per, nshards=nshards)[:2] == (total, want)


# ---- 5. code generation of the MODE 3 plain kernels ----

def unbundle(obj, d):
    d.mkdir(exist_ok=True)
    fat, co = d / "fatbin.bin", d / "k.co"
    # an explicit output file: objcopy with only an input rewrites it in place
    subprocess.check_call(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj, str(d / "copy.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    return co


def kernel_metadata(co):
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], text=True)
    out = {}
    for block in notes.split("  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        if name and vg and sp:
            out[name.group(1)] = (int(vg.group(1)), int(sp.group(1)))
    return out


def hot_loops(co, kernel):
    """(VALU instructions, address after the phase pin or None) of each straight-line run
    of >= 500 VALU instructions of the kernel: its per-nonce loop body."""
    d = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", str(co)], text=True)
    i = d.index("<" + kernel)
    j = d.index("s_endpgm", i)
    runs, cur = [], []
    for line in d[i:j].split("\n"):
        m = re.match(r"\s+([vs]_\S+|global_\S+|scratch_\S+|ds_\S+|buffer_\S+|flat_\S+)\s(.*)//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        cur.append((int(m.group(3), 16), m.group(1), m.group(2).strip()))
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            runs.append(cur)
            cur = []
    runs.append(cur)
    out = []
    for r in runs:
        valu = sum(1 for _, op, _ in r if op.startswith("v_"))
        if valu < 500:
            continue
        pin = None
        for n, (addr, op, args) in enumerate(r[: max(len(r) // 10, 2)]):
            if op == "s_nop" and args == "0" and addr % 8 == 0 and n + 1 < len(r):
                pin = r[n + 1][0]
                break
        out.append((valu, pin))
    return out


def test_collect_plain_kernels_codegen(tmp_path):
    """The MODE 3 plain kernels keep what the search kernels' rate rests on (test_codegen.py,
    test_first_below_cpu.py): all 14 J present, <= 64 VGPRs (8 waves per SIMD), no spills in
    the J = 4 and J = 5 kernels, exactly one per-nonce loop body in J = 4 with no more VALU
    instructions than MODE 0's (the collecting test costs one compare and one ballot, as the
    pruning test does), opening at 4 mod 8 bytes."""
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("binutils / ROCm LLVM tools not present")
    cos = {}
    for tu in ("kernels_plain_collect", "kernels_plain"):
        obj = os.path.join(PKG, "build", tu + ".o")
        if not os.path.exists(obj):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{tu}.o"])
        cos[tu] = unbundle(obj, tmp_path / tu)
    scans = {}
    for name, v in kernel_metadata(cos["kernels_plain_collect"]).items():
        m = re.search(r"k_scanILi(\d+)ELi0ELb0ELi3E", name)
        if m:
            scans[int(m.group(1))] = v
    assert sorted(scans) == list(range(14)), scans
    for J, (vgpr, spill) in scans.items():
        assert vgpr <= 64, (J, vgpr)
    assert scans[4][1] == 0 and scans[5][1] == 0, scans
    collect = hot_loops(cos["kernels_plain_collect"], "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi3EE")
    search = hot_loops(cos["kernels_plain"], "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi0EE")
    assert len(collect) == 1 and len(search) == 1, (collect, search)
    assert collect[0][0] <= search[0][0], (collect, search)
    assert collect[0][1] is not None and collect[0][1] % 8 == 4, collect
    assert search[0][1] is not None and search[0][1] % 8 == 4, search
