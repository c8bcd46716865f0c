#!/usr/bin/env python3
"""Writes tests/golden/pq_net.npz: seeded codebooks, codes and queries and what the reference's own matching_PQ_Net
(src/utils/nnsearch.py:905-946, imported through oracle.make_golden.import_reference) returns for them.  Build container
only; needs the reference tree.

Inputs: N = 2000 codes of M = 16 books of Ks = 256 codewords, d = 128 (L = 8), Gaussian codebooks and 7 Gaussian queries,
K = 100; twenty code rows are copies of other rows, so exact ties exist.  The reference's np.argsort is not stable and its sums
are float32, so the fixture is compared tie-aware (tests/_pq_truth.tie_aware_vs_reference); the script checks that the numpy
truth satisfies that comparison before it writes the file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from oracle.make_golden import import_reference
    from _pq_truth import books_of, pq_truth, tie_aware_vs_reference
    nn = import_reference()[0]
    rng = np.random.default_rng(20240917)
    N, d, M, Ks, Q, K = 2000, 128, 16, 256, 7, 100
    codewords = rng.standard_normal((Ks, d)).astype(np.float32)
    query = rng.standard_normal((Q, d)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(N, M), dtype=np.int64)
    dup_dst = rng.choice(np.arange(1000, 2000), size=20, replace=False)
    dup_src = rng.choice(np.arange(0, 1000), size=20, replace=False)
    codes[dup_dst] = codes[dup_src]
    # two queries sit next to a duplicated row's reconstruction, so that the tied pair lands among the first K
    for qi, src in ((0, dup_src[0]), (3, dup_src[7])):
        recon = np.concatenate([codewords[codes[src, m], m * (d // M):(m + 1) * (d // M)] for m in range(M)])
        query[qi] = recon + 0.05 * rng.standard_normal(d).astype(np.float32)
    idx, _ = nn.matching_PQ_Net(K, codewords, query, M, codes)
    idx = np.asarray(idx, dtype=np.int64)
    ours, _ = pq_truth(query, books_of(codewords, M), codes, K)
    bad = tie_aware_vs_reference(idx, ours, codewords, query, M, codes)
    if bad:
        raise SystemExit("the truth disagrees with the reference: " + "; ".join(bad))
    print("positions identical to the reference: %.2f %%" % (100.0 * (idx == ours).mean()))
    out = os.path.join(ROOT, "tests", "golden", "pq_net.npz")
    np.savez_compressed(out, codewords=codewords, query=query, codes=codes.astype(np.uint8), n_books=np.int64(M), K=np.int64(K),
                        idx=idx)
    print("written", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
