"""Pure-numpy truth of mi_kmeans_train / mi_kmeans_assign (tests only).  The contract is mi_pqw_train's with one book, so the truth
is _pq_train_truth / _pq_wide_truth as they stand; this file adds the certificate of DESIGN.md 5.14g restated in numpy (tau), the
expanded form it is applied to, and the inputs of the tests."""
import numpy as np

from _pq_truth import dtable64
from _pq_train_truth import update_truth

U = 2.0 ** -53


def gamma(d):
    return (d + 3) * U / (1.0 - (d + 3) * U)


def tau_rows(x, C):
    """tau [n] of every row under centroids C [k, d]: 4 gamma (xn + cmax)^2 with xn >= ||x||, cmax >= max ||c||, every factor
    rounded up by 1 + 2^-30, plus the underflow term -- csrc/kmeans.hip's km_tau."""
    x64, C64 = np.asarray(x).astype(np.float64), np.asarray(C, np.float32).astype(np.float64)
    d = x64.shape[1]
    up = 1.0 + 2.0 ** -30
    xn = np.sqrt((x64 * x64).sum(1)) * up
    cm = np.sqrt((C64 * C64).sum(1).max()) * up
    return 4.0 * gamma(d) * (xn + cm) ** 2 * up + (d + 3) * 2.0 ** -1000


def expanded_gap(x, C):
    """second lowest - lowest of e[i][c] = ||c||^2 - 2 x_i . c in float64 (numpy's summation order, not the kernel's: the two differ
    by at most tau / 2, see flagged_cap)."""
    x64, C64 = np.asarray(x).astype(np.float64), np.asarray(C, np.float32).astype(np.float64)
    e = (C64 * C64).sum(1)[None, :] - 2.0 * (x64 @ C64.T)
    e.sort(axis=1)
    return e[:, 1] - e[:, 0]


def flagged_cap(x, C):
    """An upper bound of the rows the matrix kernel may flag: every e is within tau / 4 of the real value in ANY summation order, so
    a numpy gap above 2 tau is a kernel gap above tau."""
    return int((expanded_gap(x, C) <= 2.0 * tau_rows(x, C)).sum())


def assign_truth(x, C, block=1024):
    """-> int32 [n]: np.argmin of the float64 direct-form sums (dtable64: ascending j, one multiply and one add per term), ties to
    the lower centroid."""
    x = np.asarray(x)
    C = np.asarray(C, np.float32)[None]
    out = np.empty(x.shape[0], np.int32)
    for r in range(0, x.shape[0], block):
        out[r:r + block] = np.argmin(dtable64(x[r:r + block], C)[0][:, 0], axis=-1)
    return out


def flagged_floor(x, C):
    """A lower bound of the rows the matrix kernel must flag: a numpy gap below tau / 2 is a kernel gap below tau."""
    return int((expanded_gap(x, C) < 0.5 * tau_rows(x, C)).sum())


def train_steps(x, k, iters, C0):
    """_pq_train_truth.train_truth with one book and ids that hold k <= 8192, keeping what every iteration saw
    -> (C float32 [k, d], moved int64 [iters], caps [iterations that ran]: (flagged_floor, flagged_cap) under that iteration's
    centroids)."""
    x = np.asarray(x)
    C = np.ascontiguousarray(C0, dtype=np.float32).reshape(k, x.shape[1]).copy()
    moved = np.zeros(iters, np.int64)
    prev, caps = None, []
    for t in range(iters):
        caps.append((flagged_floor(x, C), flagged_cap(x, C)))
        ids = assign_truth(x, C)
        moved[t] = ids.size if prev is None else int((ids != prev).sum())
        if t > 0 and moved[t] == 0:
            break
        C = update_truth(x, ids[:, None], C[None])[0]
        prev = ids
    return C, moved, caps


def lattice(rng, n, k, d=17):
    """rows and centroids with coordinates in {-2 .. 2}: every sum of either form is exact, exact ties between distinct centroids
    are frequent -> (x float32 [n, d], C float32 [k, d] of distinct rows)"""
    x = rng.randint(-2, 3, (n, d)).astype(np.float32)
    C = np.unique(rng.randint(-2, 3, (4 * k, d)), axis=0)
    C = C[rng.permutation(C.shape[0])[:k]].astype(np.float32)
    assert C.shape[0] == k
    return x, C


def near_ties(d=16, scales=(0.0, 1e-3, 0.5, 2.0, 1e3)):
    """k = 2: float64 rows at the midpoint of the two centroids, displaced towards either by s * tau_row for every s
    -> (x float64 [2 * len(scales), d], C float32 [2, d])"""
    rng = np.random.RandomState(5)
    C = (rng.randn(2, d) * 3).astype(np.float32)
    C64 = C.astype(np.float64)
    mid = 0.5 * (C64[0] + C64[1])
    w = C64[1] - C64[0]
    tau = tau_rows(mid[None], C)[0]
    # moving the row by t along w changes e_1 - e_0 by -2 t ||w||^2: a displacement of the DISTANCE GAP by s tau
    rows = [mid + side * s * tau / (2.0 * (w @ w)) * w for s in scales for side in (-1.0, 1.0)]
    return np.array(rows, np.float64), C
