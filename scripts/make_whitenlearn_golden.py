#!/usr/bin/env python
"""Writes tests/golden/whitenlearn.npz: the answers of the reference's own pcawhitenlearn / whitenlearn on the inputs of
tests/_whitenlearn_inputs.py, and how far a second correct float64 implementation lies from them.

    python scripts/make_whitenlearn_golden.py --reference /path/to/reference/src [--seed 11]

The reference's src/utils/whiten.py (numpy only) is imported at run time from --reference; nothing of it is copied.  Per case
(kind in graded / gem, dtype in f64 / f32 = the input rounded to float32 and promoted back for the reference) the file holds
  m_pca, P_pca, m_sup, P_sup          the reference's outputs (the real part; the imaginary part is asserted to be exactly 0)
  dev_rows_*, dev_gram_*              distance of the CPU path of this package (whiten.pca_from_scatter /
                                      supervised_from_scatter on a numpy scatter matrix summed in chunks of 37 columns, eigh)
                                      from the reference, on sign-fixed rows of P and on P.T @ P
  dev_whitened_gram_*_<dims>          the same for the Gram matrix of the whitened columns, dims in (D, 16), absolute
plus the generator parameters (seed, D, N, N_PAIRS).  The inputs themselves are not stored: the tests rebuild them.
Conditions on the REFERENCE ALONE, checked here; the fixture is not written unless they hold (the seed is advanced until they
do): consecutive eigenvalues of both decompositions differ by a relative gap >= 1e-3; the top-10 guard (reference's 10th and
11th whitened scores closer than 1e-9) leaves out at most 1 % of the columns.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import isehr_amd  # noqa: E402,F401
from isehr_amd import whiten  # noqa: E402
import _whitenlearn_inputs as wi  # noqa: E402

DIMS = (wi.D, 16)


def load_reference(src):
    spec = importlib.util.spec_from_file_location("_ref_whiten", os.path.join(src, "utils", "whiten.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def real_exact(a, what):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        assert np.all(a.imag == 0), what + ": the reference returned a complex matrix with a non-zero imaginary part"
        a = a.real
    return np.ascontiguousarray(a, dtype=np.float64)


def one_case(ref, kind, dtype, seed):
    """-> dict of arrays, or None when the reference alone misses a condition."""
    X64, q, p = wi.make_input(kind, seed)
    X = wi.as_dtype(X64, dtype).astype(np.float64)             # what the reference computes on
    out = {}
    m_pca, P_pca = ref.pcawhitenlearn(X)
    m_sup, P_sup = ref.whitenlearn(X, q, p)
    P_pca, P_sup = real_exact(P_pca, "pcawhitenlearn"), real_exact(P_sup, "whitenlearn")
    # eigenvalue gaps of the reference's two decompositions, recomputed from its own formulas
    Xc = X - m_pca
    ev_pca = np.linalg.eigvalsh((Xc @ Xc.T + (Xc @ Xc.T).T) / (2 * X.shape[1]))
    df = X[:, q] - X[:, p]
    Pc = np.linalg.inv(ref.cholesky(df @ df.T / df.shape[1]))
    dfw = Pc @ (X - m_sup)
    Dm = dfw @ dfw.T
    ev_sup = np.linalg.eigvalsh((Dm + Dm.T) / 2)
    gap = min(wi.relative_gaps(ev_pca).min(), wi.relative_gaps(ev_sup).min())
    if gap < 1e-3:
        print("  %s/%s seed %d: smallest relative eigenvalue gap %.2e < 1e-3" % (kind, dtype, seed, gap))
        return None
    out.update(m_pca=m_pca, P_pca=P_pca, m_sup=m_sup, P_sup=P_sup, min_gap=np.float64(gap))
    # the package's CPU path on a scatter matrix summed in another order
    m1 = X.mean(axis=1, keepdims=True)
    P1, _ = whiten.pca_from_scatter(wi.chunked_scatter(X, m1), X.shape[1])
    m2 = X[:, q].mean(axis=1, keepdims=True)
    P2 = whiten.supervised_from_scatter(wi.chunked_pair_scatter(X, q, p) / q.size, wi.chunked_scatter(X, m2))
    assert np.array_equal(m1, m_pca) and np.array_equal(m2, m_sup)
    for tag, P, Pr, m in (("pca", P1, P_pca, m_pca), ("sup", P2, P_sup, m_sup)):
        out["dev_rows_" + tag] = np.float64(wi.rows_distance(P, Pr))
        out["dev_gram_" + tag] = np.float64(wi.gram_distance(P, Pr))
        for dims in DIMS:
            G = wi.whitened_gram(wi.whitenapply_numpy(X, m, P, dims))
            Gr = wi.whitened_gram(wi.whitenapply_numpy(X, m, Pr, dims))
            out["dev_whitened_gram_%s_%d" % (tag, dims)] = np.float64(np.max(np.abs(G - Gr)))
            _, _, left_out = wi.top10_sets(Gr, Gr)
            if left_out > 0.01:
                print("  %s/%s seed %d: the top-10 guard leaves out %.2f %% of the columns (%s, dims %d)"
                      % (kind, dtype, seed, 100 * left_out, tag, dims))
                return None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's src/ directory")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "whitenlearn.npz"))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    for seed in range(a.seed, a.seed + 64):
        arrays = {}
        for kind in wi.KINDS:
            for dtype in ("f64", "f32"):
                r = one_case(ref, kind, dtype, seed)
                if r is None:
                    arrays = None
                    break
                arrays.update({"%s_%s_%s" % (kind, dtype, k): v for k, v in r.items()})
            if arrays is None:
                break
        if arrays is not None:
            break
    else:
        raise SystemExit("no seed in [%d, %d) satisfies the conditions on the reference" % (a.seed, a.seed + 64))
    arrays.update(seed=np.int64(seed), D=np.int64(wi.D), N=np.int64(wi.N), N_PAIRS=np.int64(wi.N_PAIRS))
    np.savez_compressed(a.out, **arrays)
    print("seed %d -> %s (%d bytes)" % (seed, a.out, os.path.getsize(a.out)))
    for k in sorted(arrays):
        if k.split("_", 2)[-1].startswith(("dev_", "min_gap")):
            print("  %-40s %.3e" % (k, float(arrays[k])))


if __name__ == "__main__":
    main()
