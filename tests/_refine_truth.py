"""numpy float64 restatement of the shortlist re-ranking (mi_refine), the shape sweep of tests/test_gpu_refine.py
and its seeded inputs.  Shared by test_refine_cpu.py (which checks the truth itself and the sweep's tie-freeness on the host) and
test_gpu_refine.py."""
import functools

import numpy as np

KCS = [1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 8192]
DS = [1, 3, 4, 5, 255, 256, 257, 2048]
NS = [1, 65, 5000]
NQS = [1, 3, 130]
KMODES = ["one", "half", "all"]


def refine_truth(rows, q, cand, k, l2, row_offset=0):
    """rows [N, d] float32 as STORED, q [Q, d], cand int [Q, kc] global ids -> (ids int64 [Q, k], val64 float64 [Q, k]): padding
    dropped, unique ids, ((q64 - g64)^2).sum() ascending or (q64 * g64).sum() descending, lexsort by (value, id), tail -1 and
    +inf / -inf."""
    g64 = np.asarray(rows, np.float32).astype(np.float64)
    q64 = np.asarray(q, np.float32).astype(np.float64)
    cand = np.asarray(cand, np.int64)
    nq, n = cand.shape[0], g64.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    val = np.full((nq, k), np.inf if l2 else -np.inf, np.float64)
    for i in range(nq):
        c = cand[i]
        u = np.unique(c[(c >= row_offset) & (c < row_offset + n) & (c >= 0)])
        if u.size == 0:
            continue
        g = g64[u - row_offset]
        v = ((q64[i] - g) ** 2).sum(1) if l2 else (q64[i] * g).sum(1)
        order = np.lexsort((u, v if l2 else -v))[:k]
        ids[i, :order.size] = u[order]
        val[i, :order.size] = v[order]
    return ids, val


def value_bound(rows, q, ids, d, row_offset=0):
    """(d + 4) * 2^-53 * (||q||^2 + ||g||^2) per entry of ids [Q, k]; 0 at padding."""
    g64 = np.asarray(rows, np.float32).astype(np.float64)
    q64 = np.asarray(q, np.float32).astype(np.float64)
    gn = (g64 ** 2).sum(1)
    qn = (q64 ** 2).sum(1)
    ok = ids >= 0
    loc = np.where(ok, ids - row_offset, 0)
    return np.where(ok, (d + 4) * 2.0 ** -53 * (qn[:, None] + gn[loc]), 0.0)


def min_gap_over_bound(rows, q, cand, l2, row_offset=0):
    """Smallest (gap between the float64 values of two distinct candidates of one query) / (the larger of their two bounds) over
    all queries; inf when no query has two distinct candidates.  The ids of the device are pinned to the truth's only where
    this is above 2 (each side may be off by one bound)."""
    n, d = np.shape(rows)
    worst = np.inf
    for i in range(np.shape(cand)[0]):
        ids, val = refine_truth(rows, q[i:i + 1], np.asarray(cand)[i:i + 1], min(np.shape(cand)[1], n), l2, row_offset)
        m = int((ids[0] >= 0).sum())
        if m < 2:
            continue
        b = value_bound(rows, q[i:i + 1], ids, d, row_offset)[0, :m]
        gap = np.abs(np.diff(val[0, :m]))
        worst = min(worst, float((gap / np.maximum(b[1:], b[:-1])).min()))
    return worst


def sweep_cases():
    """44 cases (kc, d, N, nq, kmode, l2, row_offset) covering every value of every axis, both metrics and both kinds of offset;
    the number of queries drops where the host truth would take more than a moment (d = 1 stays on N <= 65: 5000 float32 draws
    squared collide)."""
    cases = []
    for i in range(44):
        kc = KCS[i % 11]
        d = DS[(i + i // 11 * 3) % 8]
        n = NS[(i + i // 11) % 3]
        nq = NQS[(i + i // 3) % 3]
        if d == 1 and n == 5000:
            n = 65
        while nq > 1 and nq * min(kc, n) * d > 4e7:
            nq = NQS[NQS.index(nq) - 1]
        cases.append((kc, d, n, nq, KMODES[(i + i // 11) % 3], i % 2 == 0, 0 if (i // 2) % 2 == 0 else 1000003))
    return cases


def k_of(kc, kmode):
    return {"one": 1, "half": max(1, kc // 2), "all": kc}[kmode]


@functools.lru_cache(maxsize=8)
def _rows(n, d):
    return np.random.default_rng(1000 * n + d).standard_normal((n, d)).astype(np.float32)


def case_inputs(case):
    """-> (rows f32 [N, d], q f32 [nq, d], cand int64 [nq, kc]): seeded Gaussian rows and queries; candidates drawn from
    [row_offset - 2, row_offset + N + 2), so ids below the shard, beyond it and (for row_offset 0) negative ones occur, and every
    kc > N repeats ids."""
    kc, d, n, nq, _, _, off = case
    rng = np.random.default_rng(hash((kc, d, n, nq)) % (2 ** 31))
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(off - 2, off + n + 2, size=(nq, kc)).astype(np.int64)
    return _rows(n, d), q, cand
