"""CPU: the packed kernel for tiny batch jobs (GPUHASH_LAYOUT_PACKED_ALWAYS).

No GPU here: the CPU replay of k_pack (hostcheck_min_batch and hostcheck_collect_below_batch under
the flag: the flagged stage as fill() writes it, tiles in seeded orders with several workgroups
in flight, stale reads of the per-job words, the bounded store and a short collect list, every
hash from pack.h's own block building and compression) against the oracle; the cap; the bytes of
an unflagged stage against those of the commit before the flag existed; the kernel manifest; a
stand-alone sanitizer run; and the header's statement of the flag.
"""
import ctypes
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import batch_jobs
import collect_batch_jobs
import packed_jobs
from packed_jobs import MAX_SPAN, PACKED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LIBDIR = os.path.join(PKG, "lib")
HEADER = os.path.join(ROOT, "include", "gpuhash.h")
GOLDEN_STAGE = os.path.join(ROOT, "tests", "golden", "packed_unflagged_stage.json")
GOLDEN_MANIFEST = os.path.join(ROOT, "tests", "golden", "kernel_manifest_packed.txt")
U64 = (1 << 64) - 1
u64, u32 = ctypes.c_uint64, ctypes.c_uint32
pu64 = ctypes.POINTER(u64)
MARK = 0xDEADBEEF
COLLECT_MAX = 1 << 20
FIELDS = "J C2 EX ndesc d c total nonces work_at offs_at desc_at ptab_at desc_bytes ptab_bytes".split()
# the figures DESIGN.md 3.15 records for k_pack<4> (min) and k_pack<6> (collect)
VGPRS = {4: 129, 6: 109}


def load_hostcheck(path):
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.hostcheck_set_layout_policy.argtypes = [ctypes.c_int]
    lib.hostcheck_min_batch.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int, vp, vp, vp]
    lib.hostcheck_collect_below_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, ctypes.c_int,
                                                  u64, vp, vp, vp, vp, vp]
    lib.hostcheck_stage_batch.argtypes = [vp, vp, u64, vp, vp, u32, vp, ctypes.c_int, pu64, vp, vp, u64]
    lib.hostcheck_stage_collect_batch.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, u32, vp, ctypes.c_int, pu64, vp,
                                                  vp, u64]
    return lib


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(LIBDIR, "libgpuhash_hostcheck.so")
    src = os.path.join(PKG, "csrc", "hostcheck.cpp")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", PKG, "lib/libgpuhash_hostcheck.so"])
    lib = load_hostcheck(path)
    yield lib
    lib.hostcheck_set_layout_policy(0)


def replay_min(hc, jobs, rchunk=0, policy=PACKED, order=0, batch_bytes=0, nshards=1):
    """hostcheck_min_batch: ([(hash, nonce)], (largest list fill, its bound, runs over, sub-batches))."""
    msgs, off, lower, upper = batch_jobs.flat(jobs)
    h = np.full(len(jobs), MARK, dtype=np.uint64)
    n = np.full(len(jobs), MARK, dtype=np.uint64)
    fill = np.zeros(4, dtype=np.uint64)
    rc = hc.hostcheck_min_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data, upper.ctypes.data,
                                rchunk, policy, order, batch_bytes, nshards, h.ctypes.data, n.ctypes.data,
                                fill.ctypes.data)
    assert rc == 0
    return list(zip(h.tolist(), n.tolist())), tuple(int(v) for v in fill)


def replay_collect(hc, jobs, rchunk=0, policy=PACKED, order=0, buffer=COLLECT_MAX, nshards=1):
    """hostcheck_collect_below_batch over (message, lower, upper, target, cap) jobs: ([(total, hits)],
    (largest list fill, jobs re-run, sub-batches, sub-range runs of the re-runs))."""
    msgs, off, lower, upper, target, out_off = collect_batch_jobs.flat(jobs)
    room = max(int(out_off[-1]), 1)
    x, h = np.full(room, MARK, dtype=np.uint64), np.full(room, MARK, dtype=np.uint64)
    totals = np.full(len(jobs), MARK, dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    rc = hc.hostcheck_collect_below_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data,
                                          upper.ctypes.data, target.ctypes.data, rchunk, policy, order, 0, nshards,
                                          buffer, out_off.ctypes.data, x.ctypes.data, h.ctypes.data,
                                          totals.ctypes.data, info.ctypes.data)
    assert rc == 0
    got = []
    for k, j in enumerate(jobs):
        at, held = int(out_off[k]), min(j[4], int(totals[k]))
        assert (x[at + held:at + j[4]] == MARK).all(), k
        got.append((int(totals[k]), [(int(h[at + i]), int(x[at + i])) for i in range(held)]))
    return got, tuple(int(v) for v in info)


def stage_batch(hc, jobs, policy, rchunk=0):
    """hostcheck_stage_batch under `policy`: (group rows as dicts, bytes, extra words, the buffer)."""
    msgs, off, lower, upper = batch_jobs.flat(jobs)
    hc.hostcheck_set_layout_policy(policy)
    rows = np.zeros(14 * 64, dtype=np.uint64)
    nbytes, extra = u64(0), np.zeros(8, dtype=np.uint64)
    meta = np.zeros(64 << 20, dtype=np.uint8)
    ng = hc.hostcheck_stage_batch(msgs.ctypes.data, off.ctypes.data, len(jobs), lower.ctypes.data, upper.ctypes.data,
                                  rchunk, rows.ctypes.data, 64, ctypes.byref(nbytes), extra.ctypes.data,
                                  meta.ctypes.data, meta.size)
    hc.hostcheck_set_layout_policy(0)
    assert 0 < ng <= 64 and nbytes.value <= meta.size
    groups = [dict(zip(FIELDS, (int(v) for v in rows[14 * i:14 * i + 14]))) for i in range(ng)]
    return groups, nbytes.value, [int(v) for v in extra], meta[:nbytes.value].tobytes()


# ---- 1. the class matrix ----

@pytest.fixture(scope="module")
def matrix(oracle):
    jobs = packed_jobs.matrix()
    return jobs, packed_jobs.hashes(oracle, jobs)


def test_the_matrix_reaches_every_class(matrix):
    jobs, _ = matrix
    assert 1400 <= len(jobs) <= 1600 and all(b - a + 1 in (4, 5) for _, a, b in jobs)
    classes = {(len(m) % 64, len(str(n))) for m, a, b in jobs for n in (a, b)}
    assert classes == {(o, d) for o in range(64) for d in range(1, 21)}
    # one and two tail blocks on either side of the transition, for every digit count
    blocks = {(d, 2 if o + d + 10 > 64 else 1) for o, d in classes}
    assert blocks == {(d, nb) for d in range(1, 21) for nb in (1, 2)}
    assert {len(m) for m, _, _ in jobs} >= {64, 65, 119, 120, 127, 128, 1300, 1 << 20}
    assert any(b == U64 for _, _, b in jobs)


@pytest.mark.parametrize("order", [0, 12345])
def test_class_matrix_min_matches_the_oracle(hc, matrix, order):
    jobs, hs = matrix
    got, fill = replay_min(hc, jobs, order=order)
    want = packed_jobs.expected_min(hs, jobs)
    bad = [(k, len(jobs[k][0]), jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert fill[2] == 0 and 0 < fill[0] <= fill[1], fill


@pytest.mark.parametrize("order", [1, 987654321])
def test_class_matrix_collect_matches_the_oracle(hc, matrix, order):
    jobs, hs = matrix
    targets = packed_jobs.quartile_targets(hs)
    cjobs = [(m, a, b, t, 5) for (m, a, b), t in zip(jobs, targets)]
    got, info = replay_collect(hc, cjobs, order=order)
    want = packed_jobs.expected_collect(hs, jobs, targets)
    bad = [(k, len(jobs[k][0]), jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:3]
    assert info[1] == 0 and info[0] == sum(w[0] for w in want)


# ---- 2. the shared mixes ----

@pytest.fixture(scope="module")
def mix(oracle):
    named = batch_jobs.job_mix()
    return [(m, a, b) for _, m, a, b in named], batch_jobs.expected(oracle, named)


@pytest.fixture(scope="module")
def cmix(oracle):
    return collect_batch_jobs.jobs_and_answers(oracle)


@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_min_mix_under_the_flag(hc, mix, policy, rchunk):
    jobs, want = mix
    plain, _ = replay_min(hc, jobs, rchunk, policy, 0)
    for order in (1, 12345):
        got, fill = replay_min(hc, jobs, rchunk, policy | PACKED, order)
        bad = [(k, jobs[k][1:], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (order, bad[:3])
        assert got == plain
        assert fill[2] == 0 and 0 < fill[0] <= fill[1] and fill[3] == 1, (order, fill)


@pytest.mark.parametrize("buffer", [COLLECT_MAX, 64])
@pytest.mark.parametrize("rchunk", [0, 7])
@pytest.mark.parametrize("policy", batch_jobs.POLICIES)
def test_collect_mix_under_the_flag(hc, cmix, policy, rchunk, buffer):
    jobs, want = cmix
    plain, _ = replay_collect(hc, jobs, rchunk, policy, 0, buffer)
    for order in (1, 12345):
        got, info = replay_collect(hc, jobs, rchunk, policy | PACKED, order, buffer)
        bad = [(k, jobs[k][1:], g[0], w[0]) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (order, bad[:3])
        assert got == plain
        if buffer < COLLECT_MAX:  # the short list overflowed, and the jobs it cut short were re-run
            assert info[0] == buffer and info[1] > 0 and info[3] >= info[1], (order, info)
        else:
            assert info[1] == 0 and info[0] == sum(w[0] for j, w in zip(jobs, want) if j[4]), (order, info)


def test_sub_batches_and_entries_under_the_flag(hc, mix):
    jobs, want = mix
    got, fill = replay_min(hc, jobs, 0, PACKED, 777, batch_bytes=32 * 1024, nshards=3)
    assert got == want and fill[2] == 0 and fill[3] >= 3, fill


# ---- 3. the cap ----

def test_the_cap_decides_per_job(hc):
    jobs = [(b"bradfitz", 7, 7), (b"bradfitz", 100, 100 + MAX_SPAN - 1), (b"bradfitz", 100, 100 + MAX_SPAN)]
    groups, _, _, _ = stage_batch(hc, jobs, PACKED)
    packed = [g for g in groups if g["C2"] == 4]
    scans = [g for g in groups if g["C2"] != 4]
    assert len(packed) == 1 and groups[-1] is packed[0]
    g = packed[0]
    assert (g["J"], g["EX"], g["ndesc"], g["d"]) == (U64, 0, 0, 0)  # J = -1 in a 64-bit word
    assert g["nonces"] == 1 + MAX_SPAN and g["c"] == 1
    # the job of 2^20 + 1 nonces plans to scan layouts, the same as without the flag
    plain, _, _, _ = stage_batch(hc, jobs[2:], 0)
    assert scans and sum(s["nonces"] for s in scans) == MAX_SPAN + 1
    key = lambda s: [s[f] for f in ("J", "C2", "EX", "ndesc", "d", "c", "total", "nonces")]
    assert [key(s) for s in scans] == [key(s) for s in plain]
    # tiles: [7, 7] is one of its own class; [100, 2^20 + 99] splits into 3..7 digits
    spans = [900, 9000, 90000, 900000, MAX_SPAN - 999900]
    assert g["total"] == 1 + sum(-(-s // 256) for s in spans)


# ---- 4. an unflagged stage ----

def stage_digests(lib, oracle):
    """SHA-256 of everything hostcheck_stage_batch and hostcheck_stage_collect_batch report for the
    shared mixes under every unflagged policy: group rows, sizes, extra words and the bytes."""
    jobs = [(m, a, b) for _, m, a, b in batch_jobs.job_mix()]
    cjobs, _ = collect_batch_jobs.jobs_and_answers(oracle)
    out = {}
    for policy in batch_jobs.POLICIES:
        for rchunk in (0, 7):
            groups, nbytes, extra, meta = stage_batch(lib, jobs, policy, rchunk)
            text = json.dumps([groups, nbytes, extra], sort_keys=True).encode()
            out[f"min policy={policy} rchunk={rchunk}"] = hashlib.sha256(text + meta).hexdigest()
            msgs, off, lower, upper, target, _ = collect_batch_jobs.flat(cjobs)
            lists = np.array([1 if j[4] else 0 for j in cjobs], dtype=np.uint8)
            rows = np.zeros(14 * 64, dtype=np.uint64)
            nb, ex = u64(0), np.zeros(8, dtype=np.uint64)
            buf = np.zeros(64 << 20, dtype=np.uint8)
            lib.hostcheck_set_layout_policy(policy)
            ng = lib.hostcheck_stage_collect_batch(msgs.ctypes.data, off.ctypes.data, len(cjobs), lower.ctypes.data,
                                                   upper.ctypes.data, target.ctypes.data, lists.ctypes.data, 4096,
                                                   rchunk, rows.ctypes.data, 64, ctypes.byref(nb), ex.ctypes.data,
                                                   buf.ctypes.data, buf.size)
            lib.hostcheck_set_layout_policy(0)
            assert 0 < ng <= 64
            d = hashlib.sha256(rows[:14 * ng].tobytes() + ex.tobytes() + buf[:nb.value].tobytes()).hexdigest()
            out[f"collect policy={policy} rchunk={rchunk}"] = d
    return out


def test_an_unflagged_stage_is_the_parents(hc, oracle):
    """tests/golden/packed_unflagged_stage.json holds stage_digests() of the replay library built
    from the commit before the packed kernel (python tests/test_packed_cpu.py LIB prints them):
    with the flag clear, no group, size, position or byte of a batch stage differs."""
    with open(GOLDEN_STAGE) as f:
        golden = json.load(f)
    assert len(golden) == 4 * len(batch_jobs.POLICIES)
    assert stage_digests(hc, oracle) == golden


# ---- 5. the kernel manifest ----

def _tools():
    return shutil.which("objcopy") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")


def test_the_packed_kernels_are_the_recorded_ones():
    """build/pack.o against tests/golden/kernel_manifest_packed.txt, and the figures DESIGN.md 3.15
    records: no scratch, no VGPR spill, 16 bytes of LDS, the VGPR counts.  After an intended change
    or a compiler update: python tools/kernel_manifest.py bitcoin-miner_amd/build/pack.o"""
    if not _tools():
        pytest.skip("binutils / ROCm LLVM tools not present")
    obj = os.path.join(PKG, "build", "pack.o")
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-s", "-C", PKG, "build/pack.o"])
    built = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_manifest.py"), obj], text=True)
    assert built.splitlines() == open(GOLDEN_MANIFEST).read().splitlines()
    seen = {}
    for line in built.splitlines():
        m = re.search(r"k_packILi(\d)E", line)
        f = dict(kv.split("=") for kv in line.split(" ")[2:])
        seen[int(m.group(1))] = int(f["vgpr_count"])
        assert f["private_segment_fixed_size"] == "0" and f["vgpr_spill_count"] == "0", line
        assert f["group_segment_fixed_size"] == "16", line
    assert seen == VGPRS
    # the scan kernels' manifest glob does not take the packed object
    import glob
    assert obj not in glob.glob(os.path.join(PKG, "build", "kernels*.o"))


# ---- 6. sanitizers ----

def test_packed_replay_stand_alone_under_asan_ubsan():
    """A program with its own main over the flagged replays (csrc/hostcheck_packed_main.cpp), built
    with -fsanitize=address,undefined: every message length mod 64, digit boundaries, the top of
    uint64, a job above the cap beside packed ones, sub-batches, several entries and a short
    collect list; each job checked against an ascending scan."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/hostcheck_packed_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIBDIR, "hostcheck_packed_asan")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout + r.stderr)[-4000:]


# ---- 7. the header ----

def test_the_header_states_the_flag():
    text = open(HEADER).read()
    assert re.search(r"#define\s+GPUHASH_LAYOUT_PACKED_ALWAYS\s+64\b", text)
    assert re.search(r"#define\s+GPUHASH_PACKED_MAX_SPAN\s+\(1u << 20\)", text)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+GPUHASH_LAYOUT_PACKED_ALWAYS", text, flags=re.S)
    assert m
    rule = " ".join(m.group(1).replace("*", " ").split())
    for packed in ("gpuhash_min_batch[_ex]", "gpuhash_collect_below_batch[_ex]", "at most GPUHASH_PACKED_MAX_SPAN nonces"):
        assert packed in rule, packed
    ignored = rule[rule.index("ignores it"):]
    for name in ("gpuhash_min,", "gpuhash_first_below,", "gpuhash_collect_below ", "gpuhash_first_below_batch[_ex]",
                 "gpuhash_hash_range", "gpuhash_shard_range_policy"):
        assert name in ignored, name
    assert "Results are identical with and without the flag" in rule
    assert "hosts that know their jobs are tiny" in rule
    assert "exactly as without the flag" in rule
    import gpuhash
    assert gpuhash.LAYOUT_PACKED_ALWAYS == PACKED and gpuhash.PACKED_MAX_SPAN == MAX_SPAN
    # the policy check needs no device: the flag is valid with any base and either tail flag, and
    # gpuhash_shard_range_policy ignores it
    cuts = gpuhash.shard_range(8, 0, 10 ** 12, 5)
    for policy in (PACKED, 3 | PACKED, 16 | PACKED, 2 | 32 | PACKED):
        assert gpuhash.shard_range(8, 0, 10 ** 12, 5, policy) == gpuhash.shard_range(8, 0, 10 ** 12, 5, policy & ~PACKED)
    assert gpuhash.shard_range(8, 0, 10 ** 12, 5, PACKED) == cuts
    for policy in (16 | 32 | PACKED, 128, 4 | PACKED):
        with pytest.raises(gpuhash.GpuHashError):
            gpuhash.shard_range(8, 0, 10 ** 12, 5, policy)
    # no new exported symbol: the flag rides on gpuhash_set_layout_policy
    assert not [s for s in gpuhash.EXPORTED if "pack" in s]


if __name__ == "__main__":  # the digests of a replay library, for tests/golden/packed_unflagged_stage.json
    sys.path[:0] = [os.path.join(ROOT, "oracle"), PKG]
    import hash_oracle
    print(json.dumps(stage_digests(load_hostcheck(sys.argv[1]), hash_oracle.load_c_oracle()), indent=1, sort_keys=True))
