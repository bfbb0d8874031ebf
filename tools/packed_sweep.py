#!/usr/bin/env python3
"""Packed against unpacked batch calls by job size: N jobs [0, S-1] over distinct 8-byte
messages, S from 10^2 to 10^6 (fewer jobs at the large sizes), through min_batch and
count_below_batch, with and without GPUHASH_LAYOUT_PACKED_ALWAYS.  Per (S, call, policy) one JSON
line: the median wall time and kernel_ms of five calls after a warm-up, and the GH/s of each.
The table and the crossover span go into DESIGN.md 3.15; a later AUTO rule is set from them.

  python tools/packed_sweep.py [--out profiles/packed_sweep.jsonl] [--spans 100,1000,...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitcoin-miner_amd"))

SPANS = [100, 300, 1000, 3000, 10000, 30000, 100000, 300000, 1000000]


def jobs_for(span: int) -> int:
    """1,024 jobs while that is at most 2^25 nonces, then fewer; 32 at least."""
    return max(32, min(1024, (1 << 25) // span))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_sweep.jsonl"))
    ap.add_argument("--spans", default=",".join(str(s) for s in SPANS))
    args = ap.parse_args()
    import gpuhash
    rows = []
    with gpuhash.Engine([0]) as eng:
        for span in [int(s) for s in args.spans.split(",")]:
            n = jobs_for(span)
            jobs = [(b"job-%04d" % k, 0, span - 1) for k in range(n)]
            cjobs = [j + (1 << 54,) for j in jobs]  # about one hit in a thousand nonces
            calls = {"min_batch": lambda: eng.min_batch(jobs), "count_below_batch": lambda: eng.count_below_batch(cjobs)}
            for name, call in calls.items():
                answers = {}
                for label, policy in (("unflagged", gpuhash.LAYOUT_AUTO), ("packed", gpuhash.LAYOUT_PACKED_ALWAYS)):
                    eng.set_layout_policy(policy)
                    answers[label] = call()  # warm-up
                    wall, kern = [], []
                    for _ in range(5):
                        t = time.perf_counter()
                        call()
                        wall.append(time.perf_counter() - t)
                        kern.append(eng.stats()["kernel_ms"])
                    w, k = statistics.median(wall) * 1e3, statistics.median(kern)
                    row = {"span": span, "jobs": n, "call": name, "policy": label, "wall_ms": round(w, 4),
                           "kernel_ms": round(k, 4), "launches": eng.stats()["launches"],
                           "wall_GHs": round(span * n / w / 1e6, 3), "kernel_GHs": round(span * n / k / 1e6, 3)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                eng.set_layout_policy(gpuhash.LAYOUT_AUTO)
                assert answers["unflagged"] == answers["packed"], (span, name)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
