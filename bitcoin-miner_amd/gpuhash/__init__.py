"""gpuhash -- Python host-side mirror of the reference's hot-path interface.

The product is the C-ABI library ``lib/libgpuhash.so`` (include/gpuhash.h) with the
gfx950 HIP kernels.  This module is a thin ctypes binding over it that mirrors the Go
names of the reference so tests and bench read like the reference's own code:

  reference (mohitreddy1996/BitCoin-Miner)                 here
  bitcoin.Hash(msg, nonce)       bitcoin/hash.go:11-15      Hash(msg, nonce)
  bitcoin.Message/MsgType        bitcoin/message.go:8-21    Message, MsgType
  bitcoin.NewRequest/NewResult   bitcoin/message.go:25-42   NewRequest, NewResult
  bitcoin.NewJoin                bitcoin/message.go:45-47   NewJoin
  miner loop (spec'd, stubbed)   bitcoin/miner/miner.go:15  Miner.handle(request)
                                 p1.pdf pp.12-14

There is no CPU fallback: if the shared library or a gfx950 device is missing, the
constructors raise.  (``Hash`` for a single nonce is the host convenience
gpuhash_hash_cpu, the Go miner's optional self-check -- never used for a search.)
"""
from __future__ import annotations

import ctypes
import enum
import os
from dataclasses import dataclass

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libgpuhash.so")
# test-only build of the same sources with the hash truncated to 4 bits (ties everywhere)
TIETEST_LIB_PATH = os.path.join(PKG_DIR, "lib", "libgpuhash_tietest.so")

GPUHASH_OK = 0
GPUHASH_EINVAL = -1
GPUHASH_ENODEV = -2
GPUHASH_EHIP = -3
GPUHASH_ETOOLONG = -4
GPUHASH_ENOMEM = -5
GPUHASH_ECANCELED = -6
GPUHASH_MAX_MSG = 1 << 20
GPUHASH_COLLECT_MAX = 1 << 20
GPUHASH_BATCH_MAX_JOBS = 1 << 16
GPUHASH_BATCH_MAX_SPAN = 1 << 38
# Engine.collect_below_batch: the room of a job given without a cap.  The batch is built for sparse
# hits and its output arrays hold the sum of the jobs' caps, so the default is small.
BATCH_COLLECT_CAP = 256
LAYOUT_AUTO, LAYOUT_UNIFORM, LAYOUT_CLASSIC, LAYOUT_LANETABLE = 0, 1, 2, 3
# OR-able flags: tail-digit launches always / never (include/gpuhash.h)
LAYOUT_TAIL_ALWAYS, LAYOUT_TAIL_NEVER = 16, 32
LAYOUT_PACKED_ALWAYS = 64  # min_batch and collect_below_batch: jobs of <= PACKED_MAX_SPAN nonces run packed
PACKED_MAX_SPAN = 1 << 20
TAIL_MIN_SPAN = 1 << 33
# first_below_batch_early: the longest packed front its rule gives a job (GPUHASH_EARLY_MAX_PREFIX)
EARLY_MAX_PREFIX = 1 << 24

# Every symbol include/gpuhash.h declares (tests check the .so exports all of them).
EXPORTED = [
    "gpuhash_open", "gpuhash_ndevices", "gpuhash_device_count", "gpuhash_shard_range",
    "gpuhash_shard_range_policy",
    "gpuhash_set_layout_policy", "gpuhash_min", "gpuhash_min_ex",
    "gpuhash_first_below", "gpuhash_first_below_ex",
    "gpuhash_collect_below", "gpuhash_collect_below_ex",
    "gpuhash_min_batch", "gpuhash_min_batch_ex",
    "gpuhash_first_below_batch", "gpuhash_first_below_batch_ex", "gpuhash_first_below_batch_early",
    "gpuhash_collect_below_batch", "gpuhash_collect_below_batch_ex",
    "gpuhash_hash_range", "gpuhash_hash_cpu", "gpuhash_last_stats", "gpuhash_last_launches",
    "gpuhash_cancel", "gpuhash_resume", "gpuhash_progress",
    "gpuhash_close",
    "gpuhash_strerror", "gpuhash_version",
]


UINT64_MAX = (1 << 64) - 1
# deterministic argument errors: the same call fails the same way on any device/miner
ARGUMENT_ERRORS = (GPUHASH_EINVAL, GPUHASH_ETOOLONG)


class GpuHashError(RuntimeError):
    def __init__(self, rc: int, what: str):
        self.rc = rc
        super().__init__(f"{what}: {_lib().gpuhash_strerror(rc).decode()} (rc={rc})")

    @property
    def is_argument_error(self) -> bool:
        """True for EINVAL/ETOOLONG: retrying the job on another miner cannot succeed.
        False for device/resource errors (ENODEV/EHIP/ENOMEM) and for ECANCELED."""
        return self.rc in ARGUMENT_ERRORS


def _check_u64(name: str, v) -> int:
    """Bounds cross the ABI as uint64_t; ctypes would silently wrap anything outside
    [0, 2^64-1] (2**64+5 -> 5), so out-of-range or non-integer values are refused here."""
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not 0 <= v <= UINT64_MAX:
        raise ValueError(f"{name}={v} outside [0, 2^64-1]")
    return v


class Stats(ctypes.Structure):
    _fields_ = [
        ("nonces", ctypes.c_uint64),
        ("launches", ctypes.c_uint32),
        ("ndevices", ctypes.c_uint32),
        ("wall_ms", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("max_dev_kernel_ms", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


def compressions_per_nonce(rec: dict) -> int:
    """SHA-256 compressions one nonce of a launch costs: its `c` nonce-bearing blocks, plus
    the all-constant padding block an EX layout compresses from a per-nonce state (message
    lengths 44-53 mod 64 at 10-12 digits).  The roofline charges
    OPS_PER_BLOCK per compression; SURVEY 8(d)'s c-based figure
    undercounts an EX launch's work by half."""
    return int(rec["c"]) + (1 if rec["EX"] else 0)


class LaunchRecord(ctypes.Structure):
    """gpuhash_launch_record (include/gpuhash.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("device", "J", "C2", "EX", "digits", "c", "shard",
                                               "stream_device")] + [
        ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64),
        ("nonces", ctypes.c_uint64), ("ms", ctypes.c_double), ("sclk_mhz", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


_LIB = None


def _lib(path: str | None = None) -> ctypes.CDLL:
    """Loads libgpuhash.so (raises if it was not built: run __graft_entry__.build())."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(p)
    u64, sz, u8p = ctypes.c_uint64, ctypes.c_size_t, ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.gpuhash_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(vp)]
    lib.gpuhash_open.restype = ctypes.c_int
    lib.gpuhash_ndevices.argtypes = [vp]
    lib.gpuhash_ndevices.restype = ctypes.c_int
    lib.gpuhash_device_count.argtypes = []
    lib.gpuhash_device_count.restype = ctypes.c_int
    lib.gpuhash_shard_range.argtypes = [sz, u64, u64, ctypes.c_int, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_shard_range.restype = ctypes.c_int
    lib.gpuhash_shard_range_policy.argtypes = [sz, u64, u64, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_shard_range_policy.restype = ctypes.c_int
    lib.gpuhash_min.argtypes = [vp, u8p, sz, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_min.restype = ctypes.c_int
    lib.gpuhash_set_layout_policy.argtypes = [vp, ctypes.c_int]
    lib.gpuhash_set_layout_policy.restype = ctypes.c_int
    lib.gpuhash_min_ex.argtypes = [vp, u8p, sz, u64, u64, ctypes.c_uint32,
                                   ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_min_ex.restype = ctypes.c_int
    lib.gpuhash_first_below.argtypes = [vp, u8p, sz, u64, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                        ctypes.POINTER(ctypes.c_int)]
    lib.gpuhash_first_below.restype = ctypes.c_int
    lib.gpuhash_first_below_ex.argtypes = [vp, u8p, sz, u64, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64),
                                           ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int)]
    lib.gpuhash_first_below_ex.restype = ctypes.c_int
    lib.gpuhash_collect_below.argtypes = [vp, u8p, sz, u64, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                          sz, ctypes.POINTER(u64)]
    lib.gpuhash_collect_below.restype = ctypes.c_int
    lib.gpuhash_collect_below_ex.argtypes = [vp, u8p, sz, u64, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64),
                                             ctypes.POINTER(u64), sz, ctypes.POINTER(u64)]
    lib.gpuhash_collect_below_ex.restype = ctypes.c_int
    lib.gpuhash_min_batch.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                      ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_min_batch.restype = ctypes.c_int
    lib.gpuhash_min_batch_ex.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                         ctypes.c_uint32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_min_batch_ex.restype = ctypes.c_int
    lib.gpuhash_first_below_batch.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64),
                                              ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                              ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int)]
    lib.gpuhash_first_below_batch.restype = ctypes.c_int
    lib.gpuhash_first_below_batch_ex.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64),
                                                 ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.c_uint32,
                                                 ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                 ctypes.POINTER(ctypes.c_int)]
    lib.gpuhash_first_below_batch_ex.restype = ctypes.c_int
    if hasattr(lib, "gpuhash_first_below_batch_early"):  # an older build loaded by path has none
        lib.gpuhash_first_below_batch_early.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64),
                                                        ctypes.POINTER(u64), ctypes.POINTER(u64), u64,
                                                        ctypes.c_uint32, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                        ctypes.POINTER(ctypes.c_int)]
        lib.gpuhash_first_below_batch_early.restype = ctypes.c_int
    lib.gpuhash_collect_below_batch.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64),
                                                ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(sz),
                                                ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_collect_below_batch.restype = ctypes.c_int
    lib.gpuhash_collect_below_batch_ex.argtypes = [vp, vp, ctypes.POINTER(sz), sz, ctypes.POINTER(u64),
                                                   ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.c_uint32,
                                                   ctypes.POINTER(sz), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                   ctypes.POINTER(u64)]
    lib.gpuhash_collect_below_batch_ex.restype = ctypes.c_int
    lib.gpuhash_hash_range.argtypes = [vp, u8p, sz, u64, u64, vp]
    lib.gpuhash_hash_range.restype = ctypes.c_int
    lib.gpuhash_hash_cpu.argtypes = [u8p, sz, u64]
    lib.gpuhash_hash_cpu.restype = u64
    lib.gpuhash_last_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.gpuhash_last_stats.restype = ctypes.c_int
    lib.gpuhash_last_launches.argtypes = [vp, ctypes.POINTER(LaunchRecord), ctypes.c_int]
    lib.gpuhash_last_launches.restype = ctypes.c_int
    lib.gpuhash_cancel.argtypes = [vp]
    lib.gpuhash_cancel.restype = ctypes.c_int
    lib.gpuhash_resume.argtypes = [vp]
    lib.gpuhash_resume.restype = ctypes.c_int
    lib.gpuhash_progress.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.gpuhash_progress.restype = ctypes.c_int
    lib.gpuhash_close.argtypes = [vp]
    lib.gpuhash_close.restype = None
    lib.gpuhash_strerror.argtypes = [ctypes.c_int]
    lib.gpuhash_strerror.restype = ctypes.c_char_p
    lib.gpuhash_version.argtypes = []
    lib.gpuhash_version.restype = ctypes.c_char_p
    if path is None:
        _LIB = lib
    return lib


def build_id(lib_path: str | None = None) -> str:
    """Hash of the sources the loaded library was built from (gpuhash_version's build=)."""
    v = _lib(lib_path).gpuhash_version().decode()
    for tok in v.split():
        if tok.startswith("build="):
            return tok[len("build="):]
    return "unknown"


def device_count() -> int:
    """Visible HIP devices (gpuhash_device_count)."""
    return int(_lib().gpuhash_device_count())


def shard_range(msg_len: int, lower: int, upper: int, nshards: int,
                policy: int | None = None) -> list[tuple[int, int] | None]:
    """gpuhash_shard_range(_policy): the engine's cost-balanced contiguous partition of the
    inclusive [lower, upper] into nshards pieces (None = empty shard), priced under the
    layout `policy` (default AUTO) as gpuhash_min's own shards are.  Host-only."""
    _check_u64("lower", lower)
    _check_u64("upper", upper)
    if isinstance(nshards, bool) or not isinstance(nshards, int) or nshards < 1:
        raise ValueError(f"nshards={nshards!r} must be an int >= 1")
    lo = (ctypes.c_uint64 * nshards)()
    hi = (ctypes.c_uint64 * nshards)()
    if policy is None:
        rc = _lib().gpuhash_shard_range(int(msg_len), lower, upper, nshards, lo, hi)
    else:
        rc = _lib().gpuhash_shard_range_policy(int(msg_len), lower, upper, nshards, int(policy), lo, hi)
    if rc < 0:
        raise GpuHashError(rc, "gpuhash_shard_range")
    return [(int(a), int(b)) if a <= b else None for a, b in zip(lo, hi)]


def _bytes(msg) -> bytes:
    return msg.encode() if isinstance(msg, str) else bytes(msg)


class Engine:
    """One gpuhash context (one or more gfx950 devices)."""

    def __init__(self, devices: list[int] | None = None, lib_path: str | None = None):
        lib = self._lib = _lib(lib_path)
        ctx = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = lib.gpuhash_open(arr, len(devices), ctypes.byref(ctx))
        else:
            rc = lib.gpuhash_open(None, 0, ctypes.byref(ctx))
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_open")
        self._ctx = ctx

    @property
    def ndevices(self) -> int:
        return self._lib.gpuhash_ndevices(self._ctx)

    def set_layout_policy(self, policy: int) -> None:
        """LAYOUT_AUTO / LAYOUT_UNIFORM / LAYOUT_CLASSIC / LAYOUT_LANETABLE, optionally OR
        LAYOUT_TAIL_ALWAYS or LAYOUT_TAIL_NEVER, and LAYOUT_PACKED_ALWAYS for batches of tiny
        jobs: min_batch and collect_below_batch then pack every job of at most PACKED_MAX_SPAN
        nonces, one (job, nonce) per GPU lane (gpuhash_set_layout_policy)."""
        rc = self._lib.gpuhash_set_layout_policy(self._ctx, policy)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_set_layout_policy")

    def min(self, msg, lower: int, upper: int, rchunk: int = 0) -> tuple[int, int]:
        """argmin over inclusive [lower, upper] of (Hash(msg, n), n).  Bounds outside
        [0, 2^64-1] raise ValueError; lower > upper raises GpuHashError(EINVAL)."""
        _check_u64("lower", lower)
        _check_u64("upper", upper)
        if isinstance(rchunk, bool) or not isinstance(rchunk, int) or not 0 <= rchunk < 1 << 32:
            raise ValueError(f"rchunk={rchunk!r} outside [0, 2^32)")
        m = _bytes(msg)
        h, n = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._lib.gpuhash_min_ex(self._ctx, m, len(m), lower, upper, rchunk,
                                   ctypes.byref(h), ctypes.byref(n))
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_min")
        return int(h.value), int(n.value)

    def min_batch(self, jobs, rchunk: int = 0) -> list[tuple[int, int]]:
        """[(hash, nonce)] of many independent searches in one call: entry k is what
        min(*jobs[k]) returns, for jobs given as (msg, lower, upper) (gpuhash_min_batch_ex; one
        scan launch per kernel variant among all the jobs, not per job).  Checked before calling
        in: at least one and at most GPUHASH_BATCH_MAX_JOBS jobs, bounds as for min(), lower <=
        upper, at most GPUHASH_BATCH_MAX_SPAN nonces and GPUHASH_MAX_MSG message bytes per job
        (ValueError)."""
        n, data, off, lower, upper, _ = self._batch_arrays(jobs, rchunk, 3)
        hashes, nonces = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        rc = self._lib.gpuhash_min_batch_ex(self._ctx, ctypes.addressof(data), off, n, lower, upper, rchunk,
                                            hashes, nonces)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_min_batch")
        return list(zip(hashes, nonces))

    @staticmethod
    def _batch_arrays(jobs, rchunk, fields):
        """The batch calls' checks and flat arrays, for jobs of `fields` fields: (msg, lower,
        upper), then a target when there are 4.  (njobs, msgs, msg_off, lower, upper, target)."""
        what = "(msg, lower, upper)" if fields == 3 else "(msg, lower, upper, target)"
        jobs = [tuple(j) for j in jobs]
        if not 1 <= len(jobs) <= GPUHASH_BATCH_MAX_JOBS:
            raise ValueError(f"{len(jobs)} jobs outside [1, GPUHASH_BATCH_MAX_JOBS]")
        if isinstance(rchunk, bool) or not isinstance(rchunk, int) or not 0 <= rchunk < 1 << 32:
            raise ValueError(f"rchunk={rchunk!r} outside [0, 2^32)")
        msgs = []
        for k, j in enumerate(jobs):
            if len(j) != fields:
                raise ValueError(f"job {k} is not {what}")
            m, lo, hi = _bytes(j[0]), _check_u64(f"jobs[{k}].lower", j[1]), _check_u64(f"jobs[{k}].upper", j[2])
            if fields == 4:
                _check_u64(f"jobs[{k}].target", j[3])
            if lo > hi:
                raise ValueError(f"jobs[{k}]: lower={lo} > upper={hi}")
            if hi - lo >= GPUHASH_BATCH_MAX_SPAN:
                raise ValueError(f"jobs[{k}] spans more than GPUHASH_BATCH_MAX_SPAN nonces")
            if len(m) > GPUHASH_MAX_MSG:
                raise ValueError(f"jobs[{k}]: message longer than GPUHASH_MAX_MSG")
            msgs.append(m)
        n = len(jobs)
        off = (ctypes.c_size_t * (n + 1))()
        for k, m in enumerate(msgs):
            off[k + 1] = off[k] + len(m)
        data = ctypes.create_string_buffer(b"".join(msgs), off[n] + 1)
        lower = (ctypes.c_uint64 * n)(*[j[1] for j in jobs])
        upper = (ctypes.c_uint64 * n)(*[j[2] for j in jobs])
        target = (ctypes.c_uint64 * n)(*[j[3] for j in jobs]) if fields == 4 else None
        return n, data, off, lower, upper, target

    def first_below_batch(self, jobs, rchunk: int = 0) -> list[tuple[int, int] | None]:
        """Many independent first-hit searches in one call: entry k is what first_below(*jobs[k])
        returns, (hash, nonce) of the lowest nonce whose hash is <= the job's target or None, for
        jobs given as (msg, lower, upper, target) (gpuhash_first_below_batch_ex; one scan launch
        per digit count and kernel variant among all the jobs, in ascending digit order).  Jobs
        are checked before calling in, as for min_batch (ValueError, TypeError)."""
        n, data, off, lower, upper, target = self._batch_arrays(jobs, rchunk, 4)
        hashes, nonces, found = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_int * n)()
        rc = self._lib.gpuhash_first_below_batch_ex(self._ctx, ctypes.addressof(data), off, n, lower, upper, target,
                                                    rchunk, hashes, nonces, found)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_first_below_batch")
        return [(int(hashes[k]), int(nonces[k])) if found[k] else None for k in range(n)]

    def first_below_batch_early(self, jobs, prefix: int = 0, rchunk: int = 0) -> list[tuple[int, int] | None]:
        """first_below_batch for jobs whose first hit lies early in their range (stamp jobs): the
        same results, with the first nonces of every job hashed packed, one (job, nonce) per GPU
        lane, in ascending rounds of doubling pieces, and what is left of the jobs still open as
        first_below_batch runs it (gpuhash_first_below_batch_early).  prefix = 0 lets every job's
        target decide how many of its nonces run packed, at most EARLY_MAX_PREFIX; another value,
        up to GPUHASH_BATCH_MAX_SPAN, forces it (tuning).  Jobs are checked as for
        first_below_batch."""
        n, data, off, lower, upper, target = self._batch_arrays(jobs, rchunk, 4)
        if isinstance(prefix, bool) or not isinstance(prefix, int) or not 0 <= prefix <= GPUHASH_BATCH_MAX_SPAN:
            raise ValueError(f"prefix={prefix!r} outside [0, GPUHASH_BATCH_MAX_SPAN]")
        hashes, nonces, found = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_int * n)()
        rc = self._lib.gpuhash_first_below_batch_early(self._ctx, ctypes.addressof(data), off, n, lower, upper,
                                                       target, prefix, rchunk, hashes, nonces, found)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_first_below_batch_early")
        return [(int(hashes[k]), int(nonces[k])) if found[k] else None for k in range(n)]

    def first_below(self, msg, lower: int, upper: int, target: int, rchunk: int = 0) -> tuple[int, int] | None:
        """(hash, nonce) of the LOWEST nonce n of the inclusive [lower, upper] with
        Hash(msg, n) <= target -- what an ascending scan that stops at its first hit returns
        -- or None when no nonce of the range qualifies (gpuhash_first_below_ex).  Arguments
        are checked as for min()."""
        _check_u64("lower", lower)
        _check_u64("upper", upper)
        _check_u64("target", target)
        if isinstance(rchunk, bool) or not isinstance(rchunk, int) or not 0 <= rchunk < 1 << 32:
            raise ValueError(f"rchunk={rchunk!r} outside [0, 2^32)")
        m = _bytes(msg)
        h, n, found = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        rc = self._lib.gpuhash_first_below_ex(self._ctx, m, len(m), lower, upper, target, rchunk,
                                              ctypes.byref(h), ctypes.byref(n), ctypes.byref(found))
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_first_below")
        return (int(h.value), int(n.value)) if found.value else None

    def collect_below(self, msg, lower: int, upper: int, target: int, cap: int = GPUHASH_COLLECT_MAX,
                      rchunk: int = 0) -> tuple[int, list[tuple[int, int]]]:
        """(total, hits): the exact number of nonces n of the inclusive [lower, upper] with
        Hash(msg, n) <= target, and the (hash, nonce) of the LOWEST min(cap, total) of them,
        ascending by nonce (gpuhash_collect_below_ex).  Every nonce is hashed; built for sparse
        hits.  A target or a cap (0..GPUHASH_COLLECT_MAX) out of range raises ValueError; the
        other arguments are checked as for min()."""
        _check_u64("lower", lower)
        _check_u64("upper", upper)
        _check_u64("target", target)
        if isinstance(cap, bool) or not isinstance(cap, int) or not 0 <= cap <= GPUHASH_COLLECT_MAX:
            raise ValueError(f"cap={cap!r} outside [0, GPUHASH_COLLECT_MAX]")
        if isinstance(rchunk, bool) or not isinstance(rchunk, int) or not 0 <= rchunk < 1 << 32:
            raise ValueError(f"rchunk={rchunk!r} outside [0, 2^32)")
        m = _bytes(msg)
        nonces = (ctypes.c_uint64 * cap)() if cap else None
        hashes = (ctypes.c_uint64 * cap)() if cap else None
        total = ctypes.c_uint64()
        rc = self._lib.gpuhash_collect_below_ex(self._ctx, m, len(m), lower, upper, target, rchunk,
                                                nonces, hashes, cap, ctypes.byref(total))
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_collect_below")
        k = min(cap, int(total.value))
        return int(total.value), [(int(hashes[i]), int(nonces[i])) for i in range(k)]

    def count_below(self, msg, lower: int, upper: int, target: int, rchunk: int = 0) -> int:
        """How many nonces of the inclusive [lower, upper] have Hash(msg, n) <= target:
        collect_below with cap = 0, which lists nothing."""
        return self.collect_below(msg, lower, upper, target, cap=0, rchunk=rchunk)[0]

    def collect_below_batch(self, jobs, rchunk: int = 0) -> list[tuple[int, list[tuple[int, int]]]]:
        """Many independent collections in one call: entry k is what collect_below(*jobs[k]) returns,
        (total, hits), for jobs given as (msg, lower, upper, target[, cap]); a job without a cap
        has room for BATCH_COLLECT_CAP hits, and cap = 0 only counts (gpuhash_collect_below_batch_ex;
        one scan launch per kernel variant among all the jobs).  Every nonce of every job is hashed;
        built for sparse hits.  Jobs are checked before calling in, as for first_below_batch, and
        a cap as for collect_below (ValueError, TypeError)."""
        jobs = [tuple(j) for j in jobs]
        caps = []
        for k, j in enumerate(jobs):
            if len(j) not in (4, 5):
                raise ValueError(f"job {k} is not (msg, lower, upper, target[, cap])")
            cap = j[4] if len(j) == 5 else BATCH_COLLECT_CAP
            if isinstance(cap, bool) or not isinstance(cap, int):
                raise TypeError(f"jobs[{k}].cap must be an int, got {type(cap).__name__}")
            if not 0 <= cap <= GPUHASH_COLLECT_MAX:
                raise ValueError(f"jobs[{k}].cap={cap} outside [0, GPUHASH_COLLECT_MAX]")
            caps.append(cap)
        n, data, off, lower, upper, target = self._batch_arrays([j[:4] for j in jobs], rchunk, 4)
        out_off = (ctypes.c_size_t * (n + 1))()
        for k, cap in enumerate(caps):
            out_off[k + 1] = out_off[k] + cap
        room = out_off[n]
        nonces = (ctypes.c_uint64 * room)() if room else None
        hashes = (ctypes.c_uint64 * room)() if room else None
        totals = (ctypes.c_uint64 * n)()
        rc = self._lib.gpuhash_collect_below_batch_ex(self._ctx, ctypes.addressof(data), off, n, lower, upper,
                                                      target, rchunk, out_off, nonces, hashes, totals)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_collect_below_batch")
        out = []
        for k in range(n):
            at, held = out_off[k], min(caps[k], int(totals[k]))
            out.append((int(totals[k]), [(int(hashes[at + i]), int(nonces[at + i])) for i in range(held)]))
        return out

    def count_below_batch(self, jobs, rchunk: int = 0) -> list[int]:
        """How many nonces of each job's range have a hash <= its target, for jobs given as (msg,
        lower, upper, target): collect_below_batch with no room at all (a null out_off), which
        lists nothing."""
        n, data, off, lower, upper, target = self._batch_arrays(jobs, rchunk, 4)
        totals = (ctypes.c_uint64 * n)()
        rc = self._lib.gpuhash_collect_below_batch_ex(self._ctx, ctypes.addressof(data), off, n, lower, upper,
                                                      target, rchunk, None, None, None, totals)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_collect_below_batch")
        return [int(t) for t in totals]

    def hash_range(self, msg, lower: int, count: int):
        """numpy uint64 array of Hash(msg, lower + i), computed by the scan kernels."""
        import numpy as np
        _check_u64("lower", lower)
        _check_u64("count", count)
        m = _bytes(msg)
        out = np.empty(count, dtype=np.uint64)
        rc = self._lib.gpuhash_hash_range(self._ctx, m, len(m), lower, count, out.ctypes.data)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_hash_range")
        return out

    def stats(self) -> dict:
        s = Stats()
        self._lib.gpuhash_last_stats(self._ctx, ctypes.byref(s))
        return s.as_dict()

    def launches(self) -> list[dict]:
        """Per-launch records (variant, nonces, HIP-event ms) of the last call."""
        n = self._lib.gpuhash_last_launches(self._ctx, None, 0)
        arr = (LaunchRecord * max(n, 1))()
        n = self._lib.gpuhash_last_launches(self._ctx, arr, n)
        return [arr[i].as_dict() for i in range(n)]

    def cancel(self) -> None:
        """Stops the search in flight on this engine, from any thread, and every search after it
        until resume(): they raise GpuHashError with rc == GPUHASH_ECANCELED (gpuhash_cancel: a
        latch, one atomic store)."""
        rc = self._lib.gpuhash_cancel(self._ctx)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_cancel")

    def resume(self) -> None:
        """Clears the cancel latch: searches started from now on run normally (gpuhash_resume)."""
        rc = self._lib.gpuhash_resume(self._ctx)
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_resume")

    def progress(self) -> tuple[int, int]:
        """(done, total) nonces of the search in flight, from any thread: total its nonce count,
        done an estimate of those handed out to the device, which never decreases within a call;
        (0, 0) with no search in flight (gpuhash_progress)."""
        done, total = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._lib.gpuhash_progress(self._ctx, ctypes.byref(done), ctypes.byref(total))
        if rc != GPUHASH_OK:
            raise GpuHashError(rc, "gpuhash_progress")
        return int(done.value), int(total.value)

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.gpuhash_close(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- mirror of the reference's bitcoin package (bitcoin/message.go, hash.go) ----

class MsgType(enum.IntEnum):
    """bitcoin/message.go:8-12 (iota order)."""
    Join = 0
    Request = 1
    Result = 2


@dataclass
class Message:
    """bitcoin.Message, message.go:16-21 (JSON field names match Go's)."""
    Type: MsgType
    Data: str = ""
    Lower: int = 0
    Upper: int = 0
    Hash: int = 0
    Nonce: int = 0

    def to_json(self) -> dict:
        return {"Type": int(self.Type), "Data": self.Data, "Lower": self.Lower,
                "Upper": self.Upper, "Hash": self.Hash, "Nonce": self.Nonce}

    def __str__(self) -> str:  # Message.String, message.go:49-60
        if self.Type == MsgType.Request:
            return f"[Request {self.Data} {self.Lower} {self.Upper}]"
        if self.Type == MsgType.Result:
            return f"[Result {self.Hash} {self.Nonce}]"
        return "[Join]"


def NewRequest(data: str, lower: int, upper: int) -> Message:  # message.go:25-32
    return Message(MsgType.Request, Data=data, Lower=lower, Upper=upper)


def NewResult(hash_: int, nonce: int) -> Message:  # message.go:36-42
    return Message(MsgType.Result, Hash=hash_, Nonce=nonce)


def NewJoin() -> Message:  # message.go:45-47
    return Message(MsgType.Join)


def Hash(msg, nonce: int) -> int:
    """bitcoin.Hash(msg, nonce), hash.go:11-15 (one nonce, host)."""
    m = _bytes(msg)
    return int(_lib().gpuhash_hash_cpu(m, len(m), _check_u64("nonce", nonce)))


class Miner:
    """The miner's Request -> Result step (miner.go:15 TODO; p1.pdf pp.13-14), on GPU.

    Go strings are byte strings: Data is hashed as its UTF-8 bytes, as
    []byte(fmt.Sprintf("%s %d", ...)) does (hash.go:13).
    """

    def __init__(self, devices: list[int] | None = None, engine: Engine | None = None):
        self.engine = engine or Engine(devices)

    def handle(self, req: Message) -> Message:
        if req.Type != MsgType.Request:
            raise ValueError(f"miner expects a Request, got {req}")
        h, n = self.engine.min(req.Data, req.Lower, req.Upper)
        return NewResult(h, n)
