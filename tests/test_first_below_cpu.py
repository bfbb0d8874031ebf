"""CPU: gpuhash_first_below -- the lowest nonce of a range whose hash is at or below a target.

No GPU here: the ABI's argument checks, the CPU replay of the kernel's first-hit mode
(hostcheck_first_below: the same plan, pieces, masks, lower-bound function and skip rule,
with the order in which workgroups take pieces chosen by a seed) against the oracle, the
lower-bound function on its own, and the code generation of the MODE 2 plain kernels.
Expected values come from oracle.hash_range + numpy: the first index with hash <= target.
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


# ---- 1. ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libgpuhash.so")):
        subprocess.check_call(["make", "-C", PKG, "-j4", "lib/libgpuhash.so"])
    import gpuhash
    return gpuhash._lib()


def test_header_declares_and_library_exports_first_below(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgpuhash.so")], text=True)
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    for f in ("gpuhash_first_below", "gpuhash_first_below_ex"):
        assert re.search(r"\bint\s+" + f + r"\s*\(", src), f
        assert f in exported, f  # unmangled extern "C"
        assert hasattr(lib, f)
    import gpuhash
    assert {"gpuhash_first_below", "gpuhash_first_below_ex"} <= set(gpuhash.EXPORTED)
    assert hasattr(gpuhash.Engine, "first_below")


def test_first_below_argument_errors_need_no_device(lib):
    import gpuhash
    h, n, f = u64(), u64(), ctypes.c_int()
    ctx = ctypes.c_void_p(1)  # never dereferenced: every check below precedes any use of it
    bh, bn, bf = ctypes.byref(h), ctypes.byref(n), ctypes.byref(f)
    assert lib.gpuhash_first_below(None, b"x", 1, 0, 1, 5, bh, bn, bf) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below_ex(None, b"x", 1, 0, 1, 5, 0, bh, bn, bf) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below(ctx, b"x", 1, 0, 1, 5, None, bn, bf) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below(ctx, b"x", 1, 0, 1, 5, bh, None, bf) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below(ctx, b"x", 1, 0, 1, 5, bh, bn, None) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below(ctx, b"x", 1, 2, 1, 5, bh, bn, bf) == gpuhash.GPUHASH_EINVAL
    assert lib.gpuhash_first_below_ex(ctx, b"x", 1, 2, 1, 5, 7, bh, bn, bf) == gpuhash.GPUHASH_EINVAL
    big = bytes(gpuhash.GPUHASH_MAX_MSG + 1)
    assert lib.gpuhash_first_below(ctx, big, len(big), 0, 1, 5, bh, bn, bf) == gpuhash.GPUHASH_ETOOLONG
    assert lib.gpuhash_first_below_ex(ctx, big, len(big), 0, 1, 5, 0, bh, bn, bf) == gpuhash.GPUHASH_ETOOLONG


def test_version_minor_is_bumped(lib):
    m = re.match(rb"gpuhash (\d+)\.(\d+) gfx950 build=", lib.gpuhash_version())
    assert m and (int(m.group(1)), int(m.group(2))) >= (0, 4)


# ---- 2. replay exactness, 3. the lower-bound function ----

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
    lib.hostcheck_first_below.argtypes = [cp, u64, u64, u64, u32, u64, u64, pu64, pu64,
                                          ctypes.POINTER(ctypes.c_int), pu64]
    lib.hostcheck_parts.argtypes = [cp, u64, u64, u64, u32, pu64, pu64, pu64, ctypes.c_int]
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


# (name, message length, layout policy, lower, count, the (C2, J == 0, EX) a launch must have,
#  whether strictly descending order can skip).
# Strictly descending order within one variant group never skips on its own: every later
# piece lies below every earlier one.  The bound acts across the groups of a call, which run
# one after the other on the stream, and across a tail-digit launch's ten interleaved
# descriptors.  So the digit boundaries below are ones where the kernel variant changes (two
# groups, the first with hits at the 1/64 target), and the last field says which windows
# have neither: the single-group windows at the top of uint64, where no boundary exists.
WINDOWS = [
    ("plain", 8, AUTO, 10 ** 7 - 2100, 4500, (0, False, 0), True),            # J = 3 -> 4
    ("plain-j0", 63, AUTO, 10 ** 4 - 2000, 4000, (0, True, 0), True),         # J = 0 -> 1
    ("ktab", 120, AUTO, 10 ** 11 - 1500, 4000, (1, True, 0), True),           # C2 = 1, J = 0 -> J = 1
    ("classic", 58, CLASSIC, 10 ** 9 - 2500, 5000, (1, False, 0), True),      # C2 = 1, J = 1
    ("two-word", 58, UNIFORM, 10 ** 9 - 2500, 5000, (2, False, 0), True),     # C2 = 2
    ("lane-table", 61, LANETABLE, 10 ** 6 - 2000, 4000, (3, False, 0), True),  # K+W table -> C2 = 3:
    #                                      the lane table runs second, so its own skip branch acts
    ("lane-table-first", 61, LANETABLE, 10 ** 10 - 2000, 4000, (3, False, 0), True),  # C2 = 3 -> J = 2
    ("extra-block", 42, AUTO, 10 ** 13 - 1800, 4000, (0, False, 1), True),    # EX, J = 13 -> 14
    ("tail-digit", 8, AUTO | TAIL_ALWAYS, 10 ** 11 - 1700, 4200, (0, False, 0), True),
    ("top-tail", 8, AUTO | TAIL_ALWAYS, U64 - 3999, 4000, (0, False, 0), True),
    ("top", 8, AUTO, U64 - 3999, 4000, (0, False, 0), False),
    ("top-two-blocks", 50, AUTO, U64 - 2999, 3000, None, False),
]
ORDERS = [0, 1, 12345, 987654321]  # ascending, strictly descending, two shuffles with batches


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
    """The window's minimum hash, that minus 1 (nothing qualifies), about the 1/64 and the
    1/1000 quantiles, and 2^64-1."""
    s = np.sort(h)
    return [int(s[0]), int(s[0]) - 1, int(s[len(s) // 64]), int(s[max(len(s) // 1000, 1)]), U64]


def expected(h, lo, target):
    idx = np.nonzero(h <= np.uint64(target))[0]
    return None if idx.size == 0 else (int(h[idx[0]]), lo + int(idx[0]))


def plan(hc, m, lo, hi, rchunk):
    arr = (Info * 512)()
    n = hc.gpuhash_plan_all(m, len(m), lo, hi, rchunk, arr, 512)
    assert 0 < n <= 512
    return list(arr[:n])


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("win", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_replay_is_exact_in_every_order(hc, oracle, win, rchunk):
    name, mlen, policy, lo, cnt, want_variant, descending_skips = win
    m = window_msg(name, mlen)
    hi = lo + cnt - 1
    h = window_hashes(oracle, name, m, lo, cnt)
    hc.hostcheck_set_layout_policy(policy)
    launches = plan(hc, m, lo, hi, rchunk)
    if want_variant:
        assert any((l.C2, l.J == 0, l.EX) == want_variant for l in launches), [(l.J, l.C2, l.EX) for l in launches]
    if policy & TAIL_ALWAYS:
        assert any(l.stride == 10 for l in launches)
    variants = {(l.J, l.C2, l.EX) for l in launches}
    targets = five_targets(h)
    for ti, target in enumerate(targets):
        want = expected(h, lo, target)
        assert (want is None) == (ti == 1)
        assert ti != 4 or want[1] == lo  # target 2^64-1 returns lower
        for order in ORDERS:
            gh, gn, found, skipped = u64(0xDEAD), u64(0xBEEF), ctypes.c_int(-1), u64()
            assert hc.hostcheck_first_below(m, len(m), lo, hi, rchunk, target, order, ctypes.byref(gh),
                                            ctypes.byref(gn), ctypes.byref(found), ctypes.byref(skipped)) == 0
            if want is None:
                assert found.value == 0 and (gh.value, gn.value) == (0xDEAD, 0xBEEF)  # outputs untouched
                assert skipped.value == 0
            else:
                assert found.value == 1 and (gh.value, gn.value) == want, (name, rchunk, ti, order)
            # the bound must do something: descending order at the 1/64 target (see WINDOWS)
            if order == 1 and ti == 2:
                assert (len(variants) > 1 or bool(policy & TAIL_ALWAYS)) == descending_skips, variants
                assert (skipped.value > 0) == descending_skips, (name, rchunk, skipped.value, variants)
    if want_variant == (3, False, 0) and name == "lane-table":
        # the lane table is the second group here: after the first group's hits every one of
        # its parts goes through its own skip branch
        assert [l.C2 for l in launches][-1] == 3 and launches[0].C2 != 3


def test_every_layout_family_is_replayed(hc):
    """The windows above reach C2 = 0, 1 (J = 0 and J = 1), 2, 3, an extra-block kernel and
    the tail-digit launches."""
    seen = set()
    tails = False
    for name, mlen, policy, lo, cnt, _, _ in WINDOWS:
        hc.hostcheck_set_layout_policy(policy)
        for l in plan(hc, window_msg(name, mlen), lo, lo + cnt - 1, 0):
            seen.add((l.C2, min(l.J, 2), l.EX))
            tails |= l.stride == 10
    assert {(0, 2, 0), (0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)} <= seen, seen
    assert any(ex for _, _, ex in seen) and tails


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("win", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_lower_bound_function(hc, win, rchunk):
    """part_min_nonce (plan.h) for every part of every piece of the windows' plans: never
    above the smallest nonce the kernel's masks admit in the part, and the masks admit each
    nonce of the window exactly once (counts add up, every least nonce lies inside)."""
    name, mlen, policy, lo, cnt, _, _ = win
    m = window_msg(name, mlen)
    hc.hostcheck_set_layout_policy(policy)
    cap = 1 << 16
    bound, least, count = (u64 * cap)(), (u64 * cap)(), (u64 * cap)()
    n = hc.hostcheck_parts(m, len(m), lo, lo + cnt - 1, rchunk, bound, least, count, cap)
    assert 0 < n <= cap
    b, l, c = (np.frombuffer(a, dtype=np.uint64, count=n) for a in (bound, least, count))
    full = c > 0
    assert full.any() and int(c.sum()) == cnt
    assert (b[full] <= l[full]).all(), (name, rchunk, int(np.nonzero(b[full] > l[full])[0][0]))
    assert (l[full] >= np.uint64(lo)).all() and (l[full] <= np.uint64(lo + cnt - 1)).all()
    assert len(set(l[full].tolist())) == int(full.sum())  # distinct parts, distinct nonces


# ---- 4. code generation of the MODE 2 plain kernels ----

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


def test_first_hit_plain_kernels_codegen(tmp_path):
    """The MODE 2 plain kernels keep what the search kernels' rate rests on (test_codegen.py):
    <= 64 VGPRs (8 waves per SIMD), no spills in the J = 4 and J = 5 kernels, a per-nonce
    loop body with no more VALU instructions than MODE 0's (the first-hit test costs one
    compare and one ballot, as the pruning test does), opening at 4 mod 8 bytes."""
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("binutils / ROCm LLVM tools not present")
    cos = {}
    for tu in ("kernels_plain_first", "kernels_plain"):
        obj = os.path.join(PKG, "build", tu + ".o")
        if not os.path.exists(obj):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{tu}.o"])
        cos[tu] = unbundle(obj, tmp_path / tu)
    scans = {}
    for name, v in kernel_metadata(cos["kernels_plain_first"]).items():
        m = re.search(r"k_scanILi(\d+)ELi0ELb0ELi2E", name)
        if m:
            scans[int(m.group(1))] = v
    assert sorted(scans) == list(range(14)), scans
    for J, (vgpr, spill) in scans.items():
        assert vgpr <= 64, (J, vgpr)
    assert scans[4][1] == 0 and scans[5][1] == 0, scans
    first = hot_loops(cos["kernels_plain_first"], "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi2EE")
    search = hot_loops(cos["kernels_plain"], "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi0EE")
    assert len(first) == 1 and len(search) == 1, (first, search)
    assert first[0][0] <= search[0][0], (first, search)
    assert first[0][1] is not None and first[0][1] % 8 == 4, first
    assert search[0][1] is not None and search[0][1] % 8 == 4, search
