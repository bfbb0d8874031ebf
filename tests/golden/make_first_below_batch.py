#!/usr/bin/env python3
"""Generate tests/golden/first_below_batch.json -- the answers of the 256 proof-of-work jobs
that tests/test_gpu_first_below_batch.py times:

    (b"pow-%04d" % k, 0, 2^32-1, 2^48-1)  for k in 0..255

i.e. per message the LOWEST nonce whose hash is at or below 2^48-1, found by an ascending scan
with the C oracle (oracle/hash_oracle.c) in windows of 2^16 nonces, and its hash re-computed by
the hashlib restatement.  A few seconds of one core.

    python tests/golden/make_first_below_batch.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hash_oracle as ho  # noqa: E402

NJOBS, UPPER, TARGET, WINDOW = 256, (1 << 32) - 1, (1 << 48) - 1, 1 << 16


def main() -> None:
    c = ho.load_c_oracle()
    jobs = []
    for k in range(NJOBS):
        msg = b"pow-%04d" % k
        lo = 0
        while True:
            h = c.hash_range(msg, lo, min(WINDOW, UPPER - lo + 1))
            idx = np.nonzero(h <= np.uint64(TARGET))[0]
            if idx.size:
                nonce, hash_ = lo + int(idx[0]), int(h[idx[0]])
                break
            lo += WINDOW
            assert lo <= UPPER, msg
        assert ho.hash_py(msg, nonce) == hash_ <= TARGET
        jobs.append({"msg_hex": msg.hex(), "hash": hash_, "nonce": nonce})
    nonces = [j["nonce"] for j in jobs]
    out = {"generated_by": "tests/golden/make_first_below_batch.py (oracle/hash_oracle.c, winners re-hashed by "
                           "oracle/hash_oracle.py)",
           "lower": 0, "upper": UPPER, "target": TARGET, "jobs": jobs}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "first_below_batch.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {dst}: lowest answer {min(nonces)}, highest {max(nonces)}, mean {sum(nonces) / len(nonces):.0f}, "
          f"{sum(n < 100000 for n in nonces)} of at most 5 digits, {sum(n >= 100000 for n in nonces)} of 6 or more")


if __name__ == "__main__":
    main()
