"""CPU: the ledger of tests/class_windows.py -- the windows reach every (message length mod 64,
digit count) class, every compiled layout and every launch arrangement the planner can name for
such a class, and the CPU replay of every launch agrees with the oracle.

No GPU here.  Every case of the table is planned with the CPU planner (gpuhash_plan_all of
libgpuhash_hostcheck.so) under its policy run and held to conditions on the INPUTS of
tests/test_gpu_class_matrix.py.  A launch arrangement is (J, C2, EX, q, s, stride): what, with the
class, fixes loop_shift, the masks, R, R1, RQ, the padding and the digit split of a descriptor.
"""
import ctypes
import os
import random
import re

import pytest

import class_windows as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFESTS = ("kernel_manifest.txt", "kernel_manifest_collect_batch.txt")
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def hc():
    lib = cw.load_planner()
    yield lib
    lib.hostcheck_set_layout_policy(cw.AUTO)


@pytest.fixture(scope="module")
def cases(hc):
    """[(message length, window, policy run, launches)] of the whole table."""
    return [(mlen, w, run, cw.window_plan(hc, mlen, w, run)) for mlen in cw.LENGTHS for w, run in cw.run_cases(hc, mlen)]


def test_table_is_what_its_docstring_says(hc, cases):
    assert len(cw.MESSAGES) == 128 and [len(m) for m in cw.MESSAGES] == list(cw.LENGTHS)
    per_run = {run: sum(c[2] == run for c in cases) for run in cw.RUN_NAMES}
    print("cases per policy run:", per_run, "in all", len(cases))
    assert per_run == {"auto": 5760, "tail": 1508, "uniform": 342, "lanetable": 342}
    for mlen in cw.LENGTHS:
        ws = cw.WINDOWS[mlen]
        assert len(ws) == len({w.name for w in ws}) == 45
        assert sum(w.hi - w.lo + 1 for w in ws) == cw.NONCES_PER_MESSAGE == 67_800
        assert all(0 <= w.lo <= w.hi <= cw.U64 for w in ws)
        assert [sum(w.kind == k for w in ws) for k in "ABCDE"] == [1, 15, 1, 16, 12]
    assert [len(b) for b in cw.BLOCKS] == [16] * 8 and [n for b in cw.BLOCKS for n in b] == list(cw.LENGTHS)
    # the runs that are left out add nothing: CLASSIC plans as AUTO does on every window
    for mlen in cw.LENGTHS:
        for w in cw.WINDOWS[mlen]:
            classic = cw.plan(hc, cw.MESSAGES[mlen], w.lo, w.hi, cw.CLASSIC | cw.TAIL_NEVER)
            assert classic == cw.window_plan(hc, mlen, w, "auto"), (mlen, w.name)


def test_parts_of_the_gpu_matrix_hold_every_case_once(hc, cases):
    """The GPU module runs the table in parts, (message lengths, policy runs): 8 blocks of 16
    lengths under the three quick runs, and the UNIFORM run one length at a time, in two halves:
    every mode's parts hold every case once."""
    everything = sorted((mlen, w.name, run) for mlen, w, run, _ in cases)
    for mode in range(7):
        parts = cw.parts_of(mode)
        in_parts = [(mlen, w.name, run) for _, (lengths, runs, share) in parts for mlen in lengths for run in runs
                    for w in cw.part_cases(hc, mlen, run, share)]
        assert sorted(in_parts) == everything, cw.MODES[mode]
        assert len(parts) == len({name for name, _ in parts}) == 8 + 2 * 30
    assert len(cw.GPU_CASES) == 7 * 68 == len({(name, mode) for name, _, mode in cw.GPU_CASES})
    assert {mlen for mlen, _, run, _ in cases if run == "uniform"} == set(cw.UNIFORM_LENGTHS)
    assert {mlen for mlen, _, run, _ in cases if run == "lanetable"} == set(cw.UNIFORM_LENGTHS)


def test_every_d_and_e_window_holds_its_pivot(hc):
    """A D window crosses a multiple of 10^4 and an E window one of 10^8, with 300 nonces of the
    same digit count on each side; the 16 pieces tile the window."""
    for mlen in cw.LENGTHS:
        for d in range(5, 21):
            for kind, step in (("D", 10 ** 4), ("E", 10 ** 8)):
                if kind == "E" and d < 9:
                    assert f"E{d}" not in cw.WINDOW[mlen]
                    continue
                w = cw.WINDOW[mlen][f"{kind}{d}"]
                lo, hi = cw.group_of(d)
                assert w.pivot % step == 0 and lo < w.pivot < hi
                assert (w.lo, w.hi) == (w.pivot - 300, w.pivot + 299) and lo <= w.lo and w.hi <= hi
                ps = cw.pieces(w)
                assert len(ps) == 16 and ps[0][0] == w.lo and ps[-1][1] == w.hi
                assert all(b + 1 == a2 for (_, b), (a2, _) in zip(ps, ps[1:]))
                assert {b - a + 1 for a, b in ps} == {37, 38}
                assert cw.halves(w) == [(w.lo, w.pivot - 1), (w.pivot, w.hi)]


def test_all_1280_classes_are_reached(cases):
    """Under AUTO | TAIL_NEVER: a class of fewer than 10,000 nonces (up to 4 digits) is covered in
    full, every other class gets at least 2,000 nonces in at least three windows."""
    seen = {}  # class -> {(message length, window): nonces}
    for mlen, w, run, p in cases:
        if run != "auto":
            continue
        for l in p:
            assert l.stride == 1 and cw.digits(l.lo) == cw.digits(l.hi) == l.d
            seen.setdefault((mlen % 64, l.d), {}).setdefault((mlen, w.name), 0)
            seen[(mlen % 64, l.d)][(mlen, w.name)] += cw.nonces(l)
    assert sorted(seen) == [(r, d) for r in range(64) for d in range(1, 21)]
    for (r, d), wins in seen.items():
        lo, hi = cw.group_of(d)
        if d <= 4:
            # both messages of the residue hash the whole group, in window A
            assert wins == {(r, "A"): hi - lo + 1, (r + 64, "A"): hi - lo + 1}, (r, d)
        else:
            assert sum(wins.values()) >= 2000 and len(wins) >= 3, (r, d, wins)


def compiled_layouts():
    """{(J, C2, EX)} of the k_scan symbols of both kernel manifests."""
    found = set()
    for name in MANIFESTS:
        for line in open(os.path.join(GOLDEN, name)).read().splitlines():
            m = re.search(r"k_scanILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE", line.split(" ", 2)[1])
            if m:
                found.add(tuple(int(g) for g in m.groups()[:3]))
    return found


def test_cases_cover_every_compiled_layout(cases):
    seen = {cw.layout(l) for _, _, _, p in cases for l in p}
    compiled = compiled_layouts()
    assert len(compiled) == 21 and seen == compiled, (sorted(compiled - seen), sorted(seen - compiled))


def probe_ranges(d):
    """Per digit count: the bottom 2,501 nonces of the group, the top 2,501, 600 around its middle
    and [10^(d-1), 10^(d-1) + 3 * 10^8], all clipped to the group."""
    lo, hi = cw.group_of(d)
    mid = (lo + hi) // 2
    return [(lo, min(hi, lo + 2500)), (max(lo, hi - 2500), hi), (max(lo, mid - 300), min(hi, mid + 299)),
            (lo, min(hi, lo + 3 * 10 ** 8))]


def test_cases_hold_every_arrangement_the_planner_names(hc, cases):
    """The (length mod 64, digits, J, C2, EX, q, s, stride) tuples of the cases are exactly those
    the planner yields for the probe ranges, per length 0..63, digit count and each of the eight
    combinations of layout policy and tail flag."""
    mine = {(mlen % 64, l.d) + cw.arrangement(l) for mlen, _, _, p in cases for l in p}
    probe = set()
    for mlen in range(64):
        for d in range(1, 21):
            for base in (cw.AUTO, cw.UNIFORM, cw.CLASSIC, cw.LANETABLE):
                for flag in (cw.TAIL_ALWAYS, cw.TAIL_NEVER):
                    for a, b in probe_ranges(d):
                        probe |= {(mlen, l.d) + cw.arrangement(l) for l in cw.plan(hc, cw.MESSAGES[mlen], a, b, base | flag)}
    print(f"cases: {len(mine)} tuples, {len({t[2:] for t in mine})} launch arrangements;",
          f"probe: {len(probe)} tuples, {len({t[2:] for t in probe})} launch arrangements;",
          f"missing {len(probe - mine)}, not probed {len(mine - probe)}")
    assert mine == probe, (sorted(probe - mine)[:10], sorted(mine - probe)[:10])
    assert (len(mine), len({t[2:] for t in mine})) == (1579, 659)


def test_no_launch_is_a_sliver(cases):
    """Every planned launch of every case covers at least 5 nonces."""
    least = min((cw.nonces(l), mlen, w.name, run) for mlen, w, run, p in cases for l in p)
    print("smallest launch:", least)
    assert least[0] >= 5, least


def test_d_windows_carry_between_lane_values(cases):
    """Of the 2,048 D windows under AUTO, those with a launch of a plain layout (no block B-1
    compression) that covers at least two lane values: the roll-over of the loop digits with a
    carry into the lane word, inside one launch."""
    d_windows = [p for _, w, run, p in cases if run == "auto" and w.kind == "D"]
    count = sum(any(l.C2 == 0 and l.p_last > l.p_first for l in p) for p in d_windows)
    print(f"D windows with a plain launch over two lane values: {count} of {len(d_windows)}")
    assert len(d_windows) == 2048 and count >= 1800


def test_oversized_plan_is_refused_not_thrown(hc):
    """A whole 20-digit group is some 10^9 launches: the plan entry points return a negative count
    (-2)
    where an exception used to cross into the caller."""
    room = (cw.Info * 4)()
    for a, b in ((10 ** 19, cw.U64), (0, cw.U64), (10 ** 15, 10 ** 16 - 1)):
        for policy in (cw.AUTO, cw.AUTO | cw.TAIL_ALWAYS, cw.UNIFORM, cw.LANETABLE):
            hc.hostcheck_set_layout_policy(policy)
            assert hc.gpuhash_plan_count(b"bradfitz", 8, a, b, 0) == -2, (a, b, policy)
            assert hc.gpuhash_plan_all(b"bradfitz", 8, a, b, 0, room, 4) == -2, (a, b, policy)
            assert hc.hostcheck_desc_hash(b"bradfitz", 8, a, b, 0, 0, a, ctypes.byref(u64())) == -4
    hc.hostcheck_set_layout_policy(cw.AUTO)
    assert hc.gpuhash_plan_count(b"bradfitz", 8, 10 ** 19, 10 ** 19 + 3 * 10 ** 8, 0) > 0
    assert hc.gpuhash_plan_count(b"bradfitz", 8, 0, (1 << 40) - 1, 0) > 0


@pytest.mark.parametrize("block", range(8))
def test_replay_matches_the_oracle_over_the_whole_table(hc, oracle, block):
    """hostcheck_desc_hash, the CPU restatement of what a scan kernel does with a descriptor, at
    the first, the last and one seeded interior nonce of every launch of every case: all 128
    message lengths at every digit count under every policy run."""
    rng = random.Random(f"class-window replay {block}")
    out, checked = u64(), 0
    for mlen in cw.BLOCKS[block]:
        m = cw.MESSAGES[mlen]
        for w, run in cw.run_cases(hc, mlen):
            hc.hostcheck_set_layout_policy(cw.POLICY[run])
            for i, l in enumerate(cw.window_plan(hc, mlen, w, run)):
                # an interior nonce: strictly between the ends when the launch has three or more
                k = rng.randrange(1, cw.nonces(l) - 1) if cw.nonces(l) >= 3 else 0
                for n in {l.lo, l.hi, l.lo + l.stride * k}:
                    assert hc.hostcheck_desc_hash(m, mlen, w.lo, w.hi, 0, i, n, ctypes.byref(out)) == 0
                    assert out.value == oracle.hash(m, n), (cw.class_of(mlen, n), mlen, w.name, run, i, n)
                    checked += 1
    hc.hostcheck_set_layout_policy(cw.AUTO)
    assert checked > 2500
