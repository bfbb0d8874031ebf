"""GPU: the plain search kernels whose loop bodies the build re-encodes to one code phase
(csrc/phase_rewrite.h) still compute what the oracle computes.

One window per plain kernel k_scan<J,0,false,0>, J = 0..13 (the re-encoded ones and the four
the build leaves as compiled alike), chosen so that a launch starts and ends in the middle of
a row, the window crosses a digit-count boundary, and the last row of the kernel's last launch
holds fewer than 64 lane values: partial first and last rows, idle waves and idle lanes, and the
loop's first and last iteration all run.  `test_windows_are_what_they_claim` checks those
properties against the planner without a GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
HC = os.path.join(PKG, "lib", "libgpuhash_hostcheck.so")

# J -> (message, lower, upper).  A one-block message of 4J - 9 bytes puts the loop word at J
# for 9- and 10-digit nonces (1 and 2 loop digits: rows of 2,560 and 25,600 nonces); J = 2
# takes the empty message (2 and 3 loop digits).  The empty message over 3- to 6-digit nonces
# runs J = 0 (up to 4 digits, all of them loop digits) and J = 1 (5 and 6 digits).
LOW = (b"", 123, 126_030)
WINDOWS = {0: LOW, 1: LOW, 2: (b"", 10**9 - (3 * 25_600 + 3_023), 10**9 + 40_077)}
for _J in range(3, 14):
    WINDOWS[_J] = (bytes([0x60 + _J]) * (4 * _J - 9), 10**9 - 100_123, 10**9 + 79_877)


class Info(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int) for n in "J C2 EX d q s".split()]
                + [(n, ctypes.c_uint64) for n in "lo hi base".split()]
                + [(n, ctypes.c_uint32) for n in "nblocks R rchunk nrchunks p_first p_last r_first r_last".split()]
                + [(n, ctypes.c_uint32) for n in "stride tail".split()])


def plan(msg, lo, hi):
    if not os.path.exists(HC):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(HC)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    lib.gpuhash_plan_count.argtypes = [ctypes.c_char_p, u64, u64, u64, u32]
    lib.gpuhash_plan_all.argtypes = [ctypes.c_char_p, u64, u64, u64, u32, ctypes.POINTER(Info), ctypes.c_int]
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_set_layout_policy(0)  # AUTO
    n = lib.gpuhash_plan_count(msg, len(msg), lo, hi, 0)
    arr = (Info * n)()
    assert lib.gpuhash_plan_all(msg, len(msg), lo, hi, 0, arr, n) == n
    return list(arr)


def test_windows_are_what_they_claim():
    for J, (msg, lo, hi) in WINDOWS.items():
        p = plan(msg, lo, hi)
        assert 100_000 <= hi - lo + 1 <= 250_000
        assert all(l.C2 == 0 and not l.EX and l.stride == 1 for l in p), J
        assert J in {l.J for l in p} and {l.J for l in p} <= ({0, 1} if J < 2 else {J}), (J, [l.J for l in p])
        assert len({l.d for l in p}) >= 2                       # a digit-count boundary
        first, last = p[0], p[-1]
        assert 0 < first.r_first and last.r_last < last.R - 1   # starts and ends inside a row
        l = [l for l in p if l.J == J][-1]                      # the kernel's last launch of the window
        lanes_in_last_row = (l.p_last - l.p_first) % 256 + 1
        assert lanes_in_last_row < 64, (J, lanes_in_last_row)   # fewer than 64 R nonces: idle waves and lanes
    assert sorted(WINDOWS) == list(range(14))


@pytest.fixture(scope="module")
def expected(oracle):
    """(hash, nonce) of each window by the C oracle, computed once."""
    out = {}
    for J, (msg, lo, hi) in WINDOWS.items():
        if (msg, lo, hi) not in out:
            out[(msg, lo, hi)] = oracle.min(msg, lo, hi)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("J", range(14))
def test_min_matches_oracle(engine, expected, J):
    msg, lo, hi = WINDOWS[J]
    got = engine.min(msg, lo, hi)
    kernels = {(l["J"], l["C2"], l["EX"]) for l in engine.launches()}
    assert (J, 0, 0) in kernels, kernels          # the kernel under test ran
    assert got == expected[(msg, lo, hi)], (J, got)


@pytest.mark.gpu
def test_config2_kernel_keeps_the_lowest_nonce_on_ties(oracle):
    """The J = 4 window through libgpuhash_tietest.so (the hash cut to its top 4 bits, so about
    one nonce in 16 ties for the minimum): the lowest-nonce rule through the re-encoded loop."""
    import gpuhash
    if not os.path.exists(gpuhash.TIETEST_LIB_PATH):
        pytest.fail("libgpuhash_tietest.so not built (make -C bitcoin-miner_amd)")
    msg, lo, hi = WINDOWS[4]
    k = (oracle.hash_range(msg, lo, hi - lo + 1) >> np.uint64(60)) << np.uint64(32)
    i = int(np.argmin(k))  # the first occurrence is the lowest nonce
    with gpuhash.Engine(lib_path=gpuhash.TIETEST_LIB_PATH) as eng:
        assert b"TIE-TEST" in eng._lib.gpuhash_version()
        got = eng.min(msg, lo, hi)
        assert (4, 0, 0) in {(l["J"], l["C2"], l["EX"]) for l in eng.launches()}
    assert got == (int(k[i]), lo + i), got
