"""GPU: gpuhash_cancel / gpuhash_resume / gpuhash_progress on the device.

Every workload here ends on its own in about a second or less, so a cancel that does not work is
a failed assertion, never a hang; threads are joined with a timeout.

Measured on an MI355X with this file (time from cancel() to the call's return, one launch of
2^34 nonces, or a batch of 64 x 2^26): min 5.6 ms, first_below 6.0 ms, collect_below 5.6 ms,
min_batch 7.1 ms, first_below_batch 6.2 ms, collect_below_batch 6.8 ms, against 464 / 495 / 465 /
133 / 131 / 133 ms for the same calls left alone.
"""
import ctypes
import os
import re
import signal
import socket
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import batch_jobs  # noqa: E402
import collect_batch_jobs  # noqa: E402
import first_batch_jobs  # noqa: E402
import native_programs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bitcoin-miner_amd", "lib")
ECANCELED = -6
SENT = 0xA5A5A5A5A5A5A5A5
SENT_INT = 0x5A5A5A5A
U64, SZ = ctypes.c_uint64, ctypes.c_size_t
MSG = b"bradfitz"
# about 2^34 nonces inside one digit count: one launch, 0.46 s on an MI355X
BIG_LO, BIG_HI = 10 ** 10, 10 ** 10 + (1 << 34) - 1
# the batch shape DESIGN.md 3.12 measured at about 130 ms: 64 jobs of 2^26 nonces
BIG_JOBS = [(b"msg%d" % k, 10 ** 9, 10 ** 9 + (1 << 26) - 1) for k in range(64)]
MODES = ("min", "first_below", "collect_below", "min_batch", "first_below_batch", "collect_below_batch")


@pytest.fixture(scope="module")
def one():
    """One context entry on device 0: `a single launch` means the same on any machine."""
    import gpuhash
    e = gpuhash.Engine([0])
    yield e
    e.close()


def sentinels(n, ctype=U64, value=SENT):
    return (ctype * n)(*([value] * n))


def untouched(outs):
    return all(all(int(v) == (SENT_INT if a._type_ is ctypes.c_int else SENT) for v in a) for a in outs)


def raw_call(e, mode, what):
    """(fn, outs): fn() makes the ABI call of `mode` and returns its code; outs are its output
    arrays, filled with sentinels.  what: (msg, lower, upper) for the single calls (target 0 where
    there is one), a list of (msg, lower, upper) jobs for the batches."""
    lib, ctx = e._lib, e._ctx
    if mode in ("min", "first_below", "collect_below"):
        m, lo, hi = what
        h, n = sentinels(1), sentinels(1)
        if mode == "min":
            return (lambda: lib.gpuhash_min(ctx, m, len(m), lo, hi, h, n)), [h, n]
        if mode == "first_below":
            found = sentinels(1, ctypes.c_int, SENT_INT)
            return (lambda: lib.gpuhash_first_below(ctx, m, len(m), lo, hi, 0, h, n, found)), [h, n, found]
        nonces, hashes, total = sentinels(4), sentinels(4), sentinels(1)
        return (lambda: lib.gpuhash_collect_below(ctx, m, len(m), lo, hi, 0, nonces, hashes, 4, total)), \
            [nonces, hashes, total]
    if mode == "hash_range":
        m, lo, hi = what
        out = sentinels(hi - lo + 1)
        return (lambda: lib.gpuhash_hash_range(ctx, m, len(m), lo, hi - lo + 1, ctypes.addressof(out))), [out]
    fields = 3 if mode == "min_batch" else 4
    jobs = [j + (0,) for j in what] if fields == 4 else what
    k, data, off, lower, upper, target = e._batch_arrays(jobs, 0, fields)
    hashes, nonces = sentinels(k), sentinels(k)
    if mode == "min_batch":
        return (lambda: lib.gpuhash_min_batch(ctx, ctypes.addressof(data), off, k, lower, upper, hashes, nonces)), \
            [hashes, nonces]
    if mode == "first_below_batch":
        found = sentinels(k, ctypes.c_int, SENT_INT)
        return (lambda: lib.gpuhash_first_below_batch(ctx, ctypes.addressof(data), off, k, lower, upper, target,
                                                      hashes, nonces, found)), [hashes, nonces, found]
    out_off = (SZ * (k + 1))(*[2 * i for i in range(k + 1)])
    hashes, nonces, totals = sentinels(2 * k), sentinels(2 * k), sentinels(k)
    return (lambda: lib.gpuhash_collect_below_batch(ctx, ctypes.addressof(data), off, k, lower, upper, target, out_off,
                                                    nonces, hashes, totals)), [hashes, nonces, totals]


def big(mode):
    return BIG_JOBS if mode.endswith("_batch") else (MSG, BIG_LO, BIG_HI)


def run_and_cancel(e, fn):
    """Runs fn() in a thread, polls progress() every millisecond and cancels the first time
    done > 0.  (return code, wall seconds of the call, seconds from cancel() to its return,
    progress samples); the latch is cleared again."""
    out = {}

    def call():
        t = time.perf_counter()
        out["rc"] = fn()
        out["end"] = time.perf_counter()
        out["wall"] = out["end"] - t

    th = threading.Thread(target=call)
    th.start()
    samples, t_cancel = [], None
    deadline = time.perf_counter() + 20
    while th.is_alive() and time.perf_counter() < deadline:
        s = e.progress()
        samples.append(s)
        if s[0] > 0:
            t_cancel = time.perf_counter()
            e.cancel()
            break
        time.sleep(0.001)
    th.join(30)
    assert not th.is_alive(), "the call did not return"
    e.resume()
    assert t_cancel is not None, ("progress never showed work handed out", samples[-3:])
    return out["rc"], out["wall"], out["end"] - t_cancel, samples


# ---- 1. latched before the call -------------------------------------------------------------

SMALL = (MSG, 0, 9999)
SMALL_JOBS = [(MSG, 0, 9999), (b"x", 5, 5000)]


def test_latched_before_the_call_then_exact_after_resume(one, oracle):
    e = one
    e.cancel()
    try:
        for mode in MODES + ("hash_range",):
            fn, outs = raw_call(e, mode, SMALL_JOBS if mode.endswith("_batch") else SMALL)
            t = time.perf_counter()
            assert fn() == ECANCELED, mode
            assert time.perf_counter() - t < 0.05, mode  # at once: nothing was launched
            assert untouched(outs), mode
        # argument errors still win, and the calls that ignore the latch do
        h, n = sentinels(1), sentinels(1)
        assert e._lib.gpuhash_min(e._ctx, MSG, len(MSG), 5, 4, h, n) == -1
        e.set_layout_policy(0)
        e.stats(), e.launches()
    finally:
        e.resume()
    h = oracle.hash_range(MSG, 0, 10000)
    i = int(np.argmin(h))
    assert e.min(*SMALL) == (int(h[i]), i)
    assert e.first_below(MSG, 0, 9999, int(h[i])) == (int(h[i]), i)
    assert e.first_below(MSG, 0, 9999, 0) is None
    t = int(np.sort(h)[7])
    want = collect_batch_jobs.answer(h, 0, t, 4)
    assert e.collect_below(MSG, 0, 9999, t, cap=4) == want
    hx = oracle.hash_range(b"x", 5, 4996)
    ix = int(np.argmin(hx))
    assert e.min_batch(SMALL_JOBS) == [(int(h[i]), i), (int(hx[ix]), 5 + ix)]
    assert e.first_below_batch([(MSG, 0, 9999, int(h[i])), (b"x", 5, 5000, 0)]) == [(int(h[i]), i), None]
    assert e.collect_below_batch([(MSG, 0, 9999, t, 4), (b"x", 5, 5000, int(hx[ix]), 2)]) == \
        [want, (1, [(int(hx[ix]), 5 + ix)])]
    assert (e.hash_range(MSG, 0, 10000) == h).all()


# ---- 2. in-launch cancel per mode, 3. the state it leaves -----------------------------------

def exact_after(e, mode, oracle):
    """The project's small oracle-checked cases of `mode`, a collecting call with hits and a
    listing batch: all exact on a context that has just had a call cancelled."""
    named = batch_jobs.job_mix()
    cjobs, cwant = collect_batch_jobs.jobs_and_answers(oracle)
    if mode == "min":
        want = batch_jobs.expected(oracle, named)
        for (_, m, a, b), w in list(zip(named, want))[:48]:
            assert e.min(m, a, b) == w
    elif mode == "first_below":
        jobs, want = first_batch_jobs.jobs_and_answers(oracle)
        for j, w in list(zip(jobs, want))[:48]:
            assert e.first_below(*j) == w
    elif mode == "min_batch":
        assert e.min_batch([(m, a, b) for _, m, a, b in named]) == batch_jobs.expected(oracle, named)
    elif mode == "first_below_batch":
        jobs, want = first_batch_jobs.jobs_and_answers(oracle)
        assert e.first_below_batch(jobs) == want
    with_hits = [(j, w) for j, w in zip(cjobs, cwant) if w[0] > 0 and j[4] > 0]
    assert with_hits
    for j, w in with_hits[:48 if mode == "collect_below" else 6]:
        assert e.collect_below(*j) == w
    assert e.collect_below_batch(cjobs) == cwant  # a listing batch


@pytest.mark.parametrize("mode", MODES)
def test_cancel_inside_a_launch_and_the_state_it_leaves(one, oracle, mode):
    e = one
    fn, outs = raw_call(e, mode, big(mode))
    t = time.perf_counter()
    assert fn() == 0
    alone = time.perf_counter() - t
    if not mode.endswith("_batch"):
        # one launch: a pass below proves cancellation inside a launch, not at a launch boundary
        assert len(e.launches()) == 1
    fn, outs = raw_call(e, mode, big(mode))
    rc, wall, latency, samples = run_and_cancel(e, fn)
    print(f"{mode}: alone {alone * 1e3:.1f} ms, cancelled call {wall * 1e3:.1f} ms, "
          f"cancel() to return {latency * 1e3:.2f} ms, {len(samples)} progress polls")
    assert rc == ECANCELED
    assert untouched(outs)
    assert wall <= 0.5 * alone, (wall, alone)
    exact_after(e, mode, oracle)


# ---- 4. two entries on one GPU ---------------------------------------------------------------

def test_cancel_stops_both_shards_of_a_two_entry_context():
    import gpuhash
    with gpuhash.Engine([0, 0]) as e:
        fn, _ = raw_call(e, "min", big("min"))
        t = time.perf_counter()
        assert fn() == 0
        alone = time.perf_counter() - t
        assert {r["shard"] for r in e.launches()} == {0, 1}
        fn, outs = raw_call(e, "min", big("min"))
        rc, wall, latency, _ = run_and_cancel(e, fn)
        print(f"two entries: alone {alone * 1e3:.1f} ms, cancelled {wall * 1e3:.1f} ms, latency {latency * 1e3:.2f} ms")
        assert rc == ECANCELED and untouched(outs)
        assert wall <= 0.5 * alone, (wall, alone)
        assert e.min(MSG, 0, 9999) == (1419516646206828, 9898)


# ---- 5. progress -----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ("min", "min_batch"))
def test_progress_is_monotone_and_bounded(one, mode):
    e = one
    assert e.progress() == (0, 0)
    total = sum(b - a + 1 for _, a, b in BIG_JOBS) if mode == "min_batch" else BIG_HI - BIG_LO + 1
    fn, _ = raw_call(e, mode, big(mode))
    out = {}
    th = threading.Thread(target=lambda: out.update(rc=fn()))
    th.start()
    samples = []
    while th.is_alive() and len(samples) < 100000:
        samples.append(e.progress())
        time.sleep(0.002)
    th.join(30)
    assert not th.is_alive() and out["rc"] == 0
    assert e.progress() == (0, 0)
    live = [s for s in samples if s != (0, 0)]
    assert len(live) >= 5, samples[:10]
    assert all(t == total for _, t in live)
    dones = [d for d, _ in live]
    assert dones == sorted(dones) and dones[-1] <= total
    assert dones[-1] > dones[0]  # it moved while the launch was resident


# ---- 6. GPUHASH_HOST_WAIT=stream: honoured at launch boundaries ------------------------------

def test_cancel_under_stream_wait_at_a_launch_boundary(monkeypatch):
    import gpuhash
    monkeypatch.setenv("GPUHASH_HOST_WAIT", "stream")  # read when the context is opened
    monkeypatch.setenv("GPUHASH_SLICE_NONCES", str(1 << 29))  # 32 slices of ~15 ms: many launches
    with gpuhash.Engine([0]) as e:
        fn, outs = raw_call(e, "min", big("min"))
        rc, wall, _, samples = run_and_cancel(e, fn)
        assert rc == ECANCELED and untouched(outs)
        assert all(d <= t for d, t in samples)
        monkeypatch.delenv("GPUHASH_SLICE_NONCES")
        assert e.min(MSG, 0, 9999) == (1419516646206828, 9898)


# ---- 7. the C client -------------------------------------------------------------------------

def test_cli_sigint_prints_cancelled_and_exits_130():
    p = subprocess.Popen([os.path.join(LIB, "gpuhash_cli"), "bradfitz", "0", "68719476735"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    time.sleep(0.3)
    p.send_signal(signal.SIGINT)
    try:
        out, err = p.communicate(timeout=60)
    except subprocess.TimeoutExpired:
        p.kill()
        raise
    assert p.returncode == 130, (p.returncode, out, err)
    assert "Cancelled" in err and out == ""


# ---- 8. the miner ----------------------------------------------------------------------------

def test_miner_sigterm_cancels_its_job_and_the_server_requeues_it(one):
    lo, hi = 0, (1 << 36) - 1
    t = time.perf_counter()
    one.min(b"cancelme", lo, hi)
    alone = time.perf_counter() - t
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {"LSP_EPOCH_MILLIS": 100, "LSP_EPOCH_LIMIT": 5, "LSP_WINDOW_SIZE": 1}
    procs = native_programs.Procs()
    try:
        server = procs.start([os.path.join(LIB, "gpuhash_server"), str(port)],
                             dict(env, GPUHASH_JOB_SIZE=1 << 36, GPUHASH_SERVER_LOG=1))
        time.sleep(0.3)
        miner = procs.start([os.path.join(LIB, "gpuhash_miner"), f"127.0.0.1:{port}", ], dict(env, GPUHASH_DEVICES="0"))
        assert "joined" in miner.stderr.readline()  # the device is open and Join is on its way
        procs.start([os.path.join(LIB, "gpuhash_client"), f"127.0.0.1:{port}", "cancelme", str(hi)], env)
        time.sleep(0.5)  # the job has arrived and its search is in flight
        t = time.perf_counter()
        miner.send_signal(signal.SIGTERM)
        miner.wait(30)
        took = time.perf_counter() - t
        err = miner.stderr.read()
        print(f"miner: alone {alone * 1e3:.0f} ms, SIGTERM to exit {took * 1e3:.1f} ms")
        assert "signal 15" in err, err  # it was searching, and said why it leaves
        assert miner.returncode == 128 + signal.SIGTERM
        assert took <= 0.5 * alone, (took, alone)
        time.sleep(1.5)  # 5 silent epochs of 100 ms: the server notices the loss
        server.send_signal(signal.SIGTERM)
        log = server.communicate(timeout=30)[1]
        assert re.search(r"job \[\d+, \d+\] of request \d+ (requeued|still held)", log), log[-2000:]
    finally:
        procs.stop_all()
