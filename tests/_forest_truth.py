"""Plain numpy restatement of the random-projection forest (mi_forest*): projections in float64, the level-wise
build, the descent into candidate slots, and the case sweep of tests/test_gpu_forest.py.  The final order of an answer is not
restated here: it is mi_refine's, whose truth is tests/_refine_truth.py."""
import numpy as np

import _refine_truth as R  # noqa: F401  (the answer's truth; imported unchanged)

NS = [2, 64, 65, 1000, 4097]
LS = [1, 3, 6]
TS = [1, 3, 100]
DS = [1, 3, 5, 64, 130]
KMODES = ["one", "all"]
NQS = [0, 1, 65, 700]           # 700: past the 616 queries a 64 MiB chunk holds at T = 100, L = 6, leaf_max = 65
GALLERIES = ["l2", "norm_l2"]
OFFSETS = [0, 1000003]
QMODES = ["f32", "f64", "strided"]


def project(rows, dirs):
    """float64 [n, C]: P[i][c] = sum_k double(rows[i][k]) * dirs[c][k]; a sum of -0.0 is +0.0, as on the device."""
    return np.asarray(rows, np.float32).astype(np.float64) @ np.asarray(dirs, np.float64).T + 0.0


def projection_bound(rows, dirs):
    """float64 [n, C]: (d + 2) 2^-53 sum_k |x r|, the contract's bound on one projection."""
    x = np.abs(np.asarray(rows, np.float32).astype(np.float64))
    return (x.shape[1] + 2) * 2.0 ** -53 * (x @ np.abs(np.asarray(dirs, np.float64)).T)


def leaf_max(n, L):
    return -(-n // (1 << L))


def build_truth(P, T, L):
    """P float64 [n, T L] -> (splits float64 [T, 2^L - 1], leaves int32 [T, n]) as mi_forest_build defines them."""
    P = np.asarray(P, np.float64)
    n = P.shape[0]
    splits = np.zeros((T, (1 << L) - 1), np.float64)
    leaves = np.zeros((T, n), np.int32)
    for t in range(T):
        perm = np.arange(n)
        for l in range(L):
            col = P[:, t * L + l]
            for j in range(1 << l):
                a, b = (j * n) >> l, ((j + 1) * n) >> l
                seg = perm[a:b]
                seg = seg[np.lexsort((seg, col[seg]))]           # (projection, id); -0.0 == +0.0 for the comparison
                perm[a:b] = seg
                mid = ((2 * j + 1) * n) >> (l + 1)
                splits[t, (1 << l) - 1 + j] = col[seg[mid - a]]
        leaves[t] = perm
    return splits, leaves


def candidates_truth(Pq, splits, leaves, n, T, L, row_offset=0):
    """Pq float64 [Q, T L] -> int64 [Q, T leaf_max]: the leaf reached in every tree (a NaN goes left), -1 behind a short leaf."""
    Pq = np.asarray(Pq, np.float64)
    lm = leaf_max(n, L)
    out = np.full((Pq.shape[0], T * lm), -1, np.int64)
    for q in range(Pq.shape[0]):
        for t in range(T):
            j = 0
            for l in range(L):
                j = 2 * j + (1 if Pq[q, t * L + l] >= splits[t, (1 << l) - 1 + j] else 0)
            a, b = (j * n) >> L, ((j + 1) * n) >> L
            out[q, t * lm:t * lm + (b - a)] = row_offset + np.asarray(leaves[t][a:b], np.int64)
    return out


def sweep_cases():
    """24 cases (n, L, T, d, kmode, nq, gallery, row_offset, qmode) touching every value of every axis; all satisfy 2^L <= n and
    T * leaf_max <= 8192."""
    return [(2, 1, 1, 1, "one", 1, "l2", 0, "f32"),
            (2, 1, 3, 3, "all", 0, "norm_l2", 1000003, "f64"),
            (64, 1, 1, 5, "all", 65, "l2", 0, "strided"),
            (64, 3, 3, 64, "one", 1, "norm_l2", 0, "f32"),
            (64, 6, 100, 130, "all", 65, "l2", 1000003, "f64"),
            (65, 1, 3, 1, "all", 1, "l2", 0, "f64"),
            (65, 3, 100, 3, "one", 65, "norm_l2", 1000003, "strided"),
            (65, 6, 1, 5, "all", 1, "l2", 0, "f32"),
            (1000, 1, 1, 64, "one", 65, "norm_l2", 0, "f64"),
            (1000, 1, 3, 130, "all", 1, "l2", 1000003, "strided"),
            (1000, 3, 3, 1, "all", 65, "l2", 0, "f32"),
            (1000, 3, 1, 3, "one", 0, "norm_l2", 0, "f32"),
            (1000, 6, 100, 5, "all", 65, "l2", 0, "f64"),
            (1000, 6, 3, 64, "one", 1, "norm_l2", 1000003, "strided"),
            (4097, 1, 1, 130, "all", 1, "l2", 0, "f32"),
            (4097, 1, 3, 5, "one", 65, "norm_l2", 0, "f64"),
            (4097, 3, 3, 3, "all", 1, "l2", 1000003, "strided"),
            (4097, 3, 1, 64, "one", 65, "l2", 0, "f32"),
            (4097, 6, 100, 5, "all", 700, "l2", 0, "f32"),
            (4097, 6, 3, 130, "one", 65, "norm_l2", 1000003, "f64"),
            (64, 6, 3, 5, "all", 1, "norm_l2", 0, "strided"),
            (65, 1, 1, 64, "one", 0, "l2", 1000003, "f64"),
            (2, 1, 100, 130, "all", 65, "l2", 0, "strided"),
            (1000, 6, 1, 1, "one", 1, "l2", 0, "f64")]


def k_of(T, lm, kmode):
    return 1 if kmode == "one" else T * lm


def case_inputs(case):
    """-> (rows f32 [n, d], q [nq, d] in the case's dtype and layout, dirs f64 [T L, d]), all seeded.  The queries are draws of
    their own, never stored rows: a descent on given trees compares numpy's split values with the device's projections."""
    n, L, T, d, _, nq, _, _, qmode = case
    rng = np.random.default_rng(hash((n, L, T, d, nq)) % (2 ** 31))
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    dirs = rng.standard_normal((T * L, d))
    if qmode == "f64":
        q = q.astype(np.float64)
    elif qmode == "strided":
        q = np.ascontiguousarray(q.T).T                          # [nq, d] view of a [d, nq] array
    return rows, q, dirs
