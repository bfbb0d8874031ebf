"""CPU: the shared staging unit (csrc/stage.h) through hostcheck_stage -- the variant groups,
the launch metadata buffer's layout and the bytes fill() writes into it, which the engine
uploads and the CPU replays of first-hit and collect cut their pieces from.

Expected values are recomputed here from the plan (gpuhash_plan_all): grouping in
first-appearance order of (J, C2, EX), prefix offsets in row-iterations, nonce counts.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_collect_below_cpu import Info
from test_gpu_collect_below import M120, variant_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
u64, u32 = ctypes.c_uint64, ctypes.c_uint32
AUTO, UNIFORM, LANETABLE = 0, 1, 3
COUNTER_BYTES = 40  # per group: the work counter and 4 clock words
DESC_BYTES = 592    # sizeof(LaunchDesc), plan.h
# 32-bit word positions in LaunchDesc (plan.h): U, S0, CV, U1, S1, CV1, KWX are 128 words, then
# mask_lo, mask_hi, qmask, loop_shift, R, rchunk, nrchunks, p_first, p_last
DESC_R, DESC_P_FIRST, DESC_P_LAST = 132, 135, 136
FIELDS = "J C2 EX ndesc d c total nonces work_at offs_at desc_at ptab_at desc_bytes ptab_bytes".split()

# (name, msg, policy, lower, upper, the groups it plans to or None)
FORCED = [
    ("lane-table", bytes(range(61)), LANETABLE, 10 ** 6 - 1500, 10 ** 6 + 2499, [(0, 1, 0), (1, 3, 0)]),
    ("uniform", bytes(range(58)), UNIFORM, 10 ** 9 - 1500, 10 ** 9 + 2499, [(0, 1, 0), (1, 2, 0)]),
    ("empty", b"", AUTO, 0, 11999, [(0, 0, 0), (1, 0, 0)]),
    ("m120-top", M120, AUTO, 10 ** 19 - 2500, 10 ** 19 + 2499, None),
]


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(PKG, "lib", "libgpuhash_hostcheck.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = ctypes.CDLL(path)
    cp, pu64 = ctypes.c_char_p, ctypes.POINTER(u64)
    lib.gpuhash_plan_all.argtypes = [cp, u64, u64, u64, u32, ctypes.POINTER(Info), ctypes.c_int]
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_stage.argtypes = [cp, u64, u64, u64, u32, pu64, ctypes.c_int, pu64, ctypes.c_void_p, u64]
    yield lib
    lib.hostcheck_set_layout_policy(AUTO)


def plan(hc, m, lo, hi, rchunk=0):
    arr = (Info * 512)()
    n = hc.gpuhash_plan_all(m, len(m), lo, hi, rchunk, arr, 512)
    assert 0 < n <= 512
    return list(arr[:n])


def stage(hc, m, lo, hi, rchunk=0):
    """(groups as dicts of FIELDS, the metadata buffer as fill() writes it over 0xFF bytes)."""
    pu64 = ctypes.POINTER(u64)
    out = np.zeros((64, len(FIELDS)), dtype=np.uint64)
    size = u64()
    n = hc.hostcheck_stage(m, len(m), lo, hi, rchunk, out.ctypes.data_as(pu64), 64, ctypes.byref(size), None, 0)
    assert 0 < n <= 64
    meta = np.full(size.value // 8, ~np.uint64(0), dtype=np.uint64)  # 8-byte aligned, as LaunchDesc needs
    assert hc.hostcheck_stage(m, len(m), lo, hi, rchunk, out.ctypes.data_as(pu64), 64, ctypes.byref(size),
                              meta.ctypes.data, meta.nbytes) == n
    assert size.value == meta.nbytes
    return [dict(zip(FIELDS, (int(v) for v in row))) for row in out[:n]], meta.view(np.uint8)


def check_stage(hc, m, lo, hi, rchunk=0):
    launches = plan(hc, m, lo, hi, rchunk)
    groups, meta = stage(hc, m, lo, hi, rchunk)
    # groups: the first-appearance order of (J, C2, EX), each with its launches in plan order
    want = {}
    for l in launches:
        want.setdefault((l.J, l.C2, l.EX), []).append(l)
    assert [(g["J"], g["C2"], g["EX"]) for g in groups] == list(want)
    assert [g["ndesc"] for g in groups] == [len(v) for v in want.values()]
    # the counter blocks, one per group at the head of the buffer, are zeroed
    head = COUNTER_BYTES * len(groups)
    assert not meta[:head].any()
    regions = [(0, head)]
    for gi, (g, ls) in enumerate(zip(groups, want.values())):
        # prefix offsets in row-iterations, read out of the buffer
        offs = meta[g["offs_at"]:g["offs_at"] + 8 * (len(ls) + 1)].view(np.uint64).tolist()
        rows = [((l.p_last - l.p_first) // 256 + 1) * l.R for l in ls]
        assert offs == [sum(rows[:k]) for k in range(len(ls) + 1)]
        assert g["total"] == offs[-1]
        # the descriptors behind them are the group's launches, in order
        words = meta[g["desc_at"]:g["desc_at"] + g["desc_bytes"]].view(np.uint32).reshape(len(ls), DESC_BYTES // 4)
        assert g["desc_bytes"] == DESC_BYTES * len(ls)
        assert [(int(w[DESC_R]), int(w[DESC_P_FIRST]), int(w[DESC_P_LAST])) for w in words] == \
            [(l.R, l.p_first, l.p_last) for l in ls]
        # nonces, and the digits of the largest launch (the first such)
        counts = [(l.hi - l.lo) // l.stride + 1 for l in ls]
        assert g["nonces"] == sum(counts)
        assert g["d"] == ls[counts.index(max(counts))].d
        # the group's counters sit in the head block, 8-byte aligned
        assert g["work_at"] == COUNTER_BYTES * gi
        assert (g["ptab_bytes"] > 0) == (g["C2"] == 3)
        regions += [(g["offs_at"], 8 * (len(ls) + 1)), (g["desc_at"], g["desc_bytes"]), (g["ptab_at"], g["ptab_bytes"])]
    # every region is 16-byte aligned, inside the buffer, and overlaps no other
    assert all(at % 16 == 0 for at, _ in regions)
    assert regions == sorted(regions)
    assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))
    assert regions[-1][0] + regions[-1][1] <= meta.nbytes and meta.nbytes % 16 == 0
    assert sum(g["nonces"] for g in groups) == hi - lo + 1
    return groups


def test_variant_windows(hc):
    hc.hostcheck_set_layout_policy(AUTO)
    seen = set()
    for m, lo, cnt in variant_cases():
        for rchunk in (0, 7):
            seen |= {(min(g["J"], 2), g["C2"], g["EX"]) for g in check_stage(hc, m, lo, lo + cnt - 1, rchunk)}
    assert {(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 0), (2, 0, 1)} <= seen, seen


@pytest.mark.parametrize("win", FORCED, ids=[w[0] for w in FORCED])
def test_forced_windows(hc, win):
    name, m, policy, lo, hi, want = win
    hc.hostcheck_set_layout_policy(policy)
    groups = check_stage(hc, m, lo, hi)
    if want:
        assert [(g["J"], g["C2"], g["EX"]) for g in groups] == want
    if name == "empty":
        assert sum(g["ndesc"] for g in groups) == 5
    if name == "lane-table":  # the K+W-table path and the p-table path
        assert groups[0]["ptab_bytes"] == 0 and groups[1]["ptab_bytes"] > 0
