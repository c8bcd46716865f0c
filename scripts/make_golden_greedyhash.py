#!/usr/bin/env python3
"""Writes tests/golden/greedyhash.npz: seeded 0/1 hash codes and what the reference's own matching_Greedyhash
(src/utils/nnsearch.py:1001-1013, imported through oracle.make_golden.import_reference) returns for them.  Build container
only; needs the reference tree.

Inputs: 400 x 64 gallery codes, twenty rows duplicated; 7 queries, three of them copies of gallery rows; K = 10.
The reference's np.argsort is not stable, so the fixture is compared tie-aware (tests/_hamming_truth.tie_aware_equal); the
script checks that the stable numpy restatement satisfies that comparison before it writes the file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from oracle.make_golden import import_reference
    from _hamming_truth import greedyhash_restated, tie_aware_equal
    nn = import_reference()[0]
    rng = np.random.default_rng(20240611)
    train = rng.integers(0, 2, size=(400, 64), dtype=np.int64)
    dup_dst = rng.choice(np.arange(200, 400), size=20, replace=False)
    dup_src = rng.choice(np.arange(0, 200), size=20, replace=False)
    train[dup_dst] = train[dup_src]
    test = rng.integers(0, 2, size=(7, 64), dtype=np.int64)
    test[0], test[3], test[6] = train[dup_src[0]], train[17], train[399]
    K = 10
    idx, _ = nn.matching_Greedyhash(K, train, test)
    idx = np.asarray(idx, dtype=np.int64)
    ours = greedyhash_restated(K, train, test)
    bad = tie_aware_equal(idx, ours, train, test)
    if bad:
        raise SystemExit("the restatement disagrees with the reference: " + "; ".join(bad))
    out = os.path.join(ROOT, "tests", "golden", "greedyhash.npz")
    np.savez_compressed(out, train=train.astype(np.uint8), test=test.astype(np.uint8), K=np.int64(K), idx=idx)
    print("written", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
