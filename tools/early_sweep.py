#!/usr/bin/env python3
"""Sweep behind GPUHASH_EARLY_MAX_PREFIX (include/gpuhash.h).

256 stamp jobs over [0, 2^32-1] at targets 2^52-1, 2^50-1, ..., 2^40-1 -- the expected position E
of the first hit runs from 2^12 to 2^24 -- each through gpuhash_first_below_batch_early with the
prefix forced to 4 E and through gpuhash_first_below_batch, alternating in one process on one
engine; medians of five after a warm-up.  Both must give the same answers.  Writes one JSON line
per target to profiles/early_sweep.jsonl: wall time, kernel_ms, launches and packed nonces.

    python tools/early_sweep.py [--out profiles/early_sweep.jsonl] [--jobs 256] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitcoin-miner_amd"))

import gpuhash  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_sweep.jsonl"))
    ap.add_argument("--jobs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []
    with gpuhash.Engine([0]) as eng:
        for bits in range(52, 38, -2):
            target, e = (1 << bits) - 1, 1 << (64 - bits)
            prefix = min(4 * e, gpuhash.GPUHASH_BATCH_MAX_SPAN)
            jobs = [(b"pow-%04d" % k, 0, (1 << 32) - 1, target) for k in range(args.jobs)]

            def run(early):
                t = time.perf_counter()
                got = eng.first_below_batch_early(jobs, prefix) if early else eng.first_below_batch(jobs)
                wall = time.perf_counter() - t
                st = eng.stats()
                packed = sum(r["nonces"] for r in eng.launches() if r["C2"] == 4)
                return got, wall * 1e3, st["kernel_ms"], st["launches"], packed

            want = run(False)[0]
            assert run(True)[0] == want  # warm-up, and both agree
            te, tp, ke, kp = [], [], [], []
            for _ in range(args.reps):
                got, w, k, le, packed = run(True)
                assert got == want
                te.append(w)
                ke.append(k)
                got, w, k, lp, _ = run(False)
                assert got == want
                tp.append(w)
                kp.append(k)
            found = [g[1] for g in want if g]
            row = {"target_bits": bits, "E": e, "prefix": prefix, "jobs": args.jobs, "found": len(found),
                   "mean_offset": round(statistics.mean(found)) if found else None,
                   "early_ms": round(statistics.median(te), 3), "early_kernel_ms": round(statistics.median(ke), 3),
                   "early_launches": le, "packed_nonces": packed,
                   "plain_ms": round(statistics.median(tp), 3), "plain_kernel_ms": round(statistics.median(kp), 3),
                   "plain_launches": lp, "ratio": round(statistics.median(te) / statistics.median(tp), 3),
                   "version": eng._lib.gpuhash_version().decode()}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
