"""Pure-numpy truth of the Hamming radius search and self-join (tests only): distances by popcount of XOR (tests/_hamming_truth.py),
hits by (distance asc, id asc), pairs by brute force."""
import numpy as np

from _hamming_truth import hamming_distances


def distance_matrix(gallery, queries):
    """-> int32 [Q, N]: every distance, for several range_truth calls on the same codes (dmat=)."""
    gallery, queries = np.asarray(gallery, np.uint8), np.asarray(queries, np.uint8)
    out = np.empty((queries.shape[0], gallery.shape[0]), np.int32)
    for i, q in enumerate(queries):
        out[i] = hamming_distances(gallery, q)
    return out


def range_truth(gallery, queries, radius, row_offset=0, allowed=None, dmat=None):
    """-> (lims int64 [Q+1], ids int64, dist int32): per query the rows `allowed` (bool [N], None = all) admits with distance
    <= radius, ordered by np.lexsort((ids, dist)).  dmat: distance_matrix(gallery, queries) computed before."""
    if dmat is None:
        dmat = distance_matrix(gallery, queries)
    n = dmat.shape[1]
    rows = np.arange(n, dtype=np.int64) if allowed is None else np.flatnonzero(np.asarray(allowed, bool)).astype(np.int64)
    lims, ids, dist = [0], [], []
    for drow in dmat:
        d = drow[rows]
        keep = d <= radius
        r, d = rows[keep], d[keep]
        order = np.lexsort((r, d))
        ids.append(r[order] + int(row_offset))
        dist.append(d[order].astype(np.int32))
        lims.append(lims[-1] + order.size)
    return (np.asarray(lims, np.int64), np.concatenate(ids) if ids else np.empty(0, np.int64),
            np.concatenate(dist) if dist else np.empty(0, np.int32))


def pairs_truth(codes, radius):
    """-> (i int64, j int64, dist int32): all pairs i < j with distance <= radius, by i, then (distance asc, j asc)."""
    codes = np.asarray(codes, np.uint8)
    oi, oj, od = [np.empty(0, np.int64)], [np.empty(0, np.int64)], [np.empty(0, np.int32)]
    for i in range(codes.shape[0]):
        d = hamming_distances(codes[i + 1:], codes[i])
        j = np.flatnonzero(d <= radius)
        order = np.lexsort((j, d[j]))
        oi.append(np.full(order.size, i, np.int64))
        oj.append(j[order].astype(np.int64) + i + 1)
        od.append(d[j][order].astype(np.int32))
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(od)
