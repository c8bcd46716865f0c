"""Pure-numpy truth of the RESIDUAL IVF index over PQ codes (tests only), on top of _pq_truth / _ivfpq_truth: the arithmetic of
_pq_truth applied to x.astype(float64) - G[l].astype(float64), one table per (query, probed list)."""
import numpy as np

from _ivfpq_truth import probe_truth
from _pq_truth import adc_truth, dtable64, encode_truth


def residual64(x, G, lists):
    """x [N, d] float32/float64, G [nlist, d] float32, lists integer [N] -> float64 [N, d]: ONE float64 subtraction per component."""
    return np.asarray(x).astype(np.float64) - np.asarray(G, np.float32).astype(np.float64)[np.asarray(lists).astype(np.int64)]


def residual_rows_truth(x, G, lists):
    """-> float32 [N, d]: the float64 residual rounded once."""
    return residual64(x, G, lists).astype(np.float32)


def residual_encode_truth(x, G, C):
    """-> (codes uint8 [N, M], lists uint8 [N]): lists by probe_truth(x, G, 1), codes by encode_truth on the float64 residual."""
    lists = probe_truth(x, G, 1)[:, 0].astype(np.uint8)
    return encode_truth(residual64(x, G, lists), C), lists


def residual_ivfpq_truth(x, G, C, codes, lists, probes, k, row_offset=0, allowed=None):
    """probes integer [Q, P] (-1 = no list, repeats allowed) -> (ids int64 [Q, k], dist float32 [Q, k]).  Per query and distinct
    probed list l: the table dtable64(x64 - G64[l], C)[1] and adc_truth over that list's rows; the rows `allowed` admits, order by
    (distance asc, id asc), padding -1 / +inf."""
    x = np.asarray(x)
    G = np.asarray(G, np.float32)
    codes = np.asarray(codes)
    lists = np.asarray(lists).astype(np.int64)
    probes = np.asarray(probes)
    base = np.ones(lists.shape[0], bool) if allowed is None else np.asarray(allowed, bool)
    nq = x.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float32)
    members = {int(l): np.flatnonzero(base & (lists == l)).astype(np.int64) for l in np.unique(probes[probes >= 0])}
    # one dtable64 call per list over the queries that probe it
    per_query = [([], []) for _ in range(nq)]
    for l, rows in members.items():
        if rows.size == 0:
            continue
        qs = np.flatnonzero((probes == l).any(1))
        T32 = dtable64(residual64(x[qs], G, np.full(qs.size, l)), C)[1]
        d = adc_truth(T32, codes[rows])
        for t, qi in enumerate(qs):
            per_query[qi][0].append(rows)
            per_query[qi][1].append(d[t])
    for i in range(nq):
        if not per_query[i][0]:
            continue
        rows = np.concatenate(per_query[i][0])
        d = np.concatenate(per_query[i][1])
        order = np.lexsort((rows, d))[:k]
        ids[i, :order.size] = rows[order] + int(row_offset)
        dist[i, :order.size] = d[order]
    return ids, dist


def reconstruct(G, C, codes, lists, by_residual):
    """float64 [N, d]: decode(codes) (+ G[list] on a residual index)."""
    C = np.asarray(C, np.float32).astype(np.float64)
    codes = np.asarray(codes).astype(np.int64)
    out = np.concatenate([C[m, codes[:, m]] for m in range(C.shape[0])], axis=1)
    if by_residual:
        out = out + np.asarray(G, np.float32).astype(np.float64)[np.asarray(lists).astype(np.int64)]
    return out
