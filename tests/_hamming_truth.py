"""Pure-numpy truth of the Hamming search (tests only): popcount of XOR in row blocks, order by (distance, id)."""
import numpy as np

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)
INT32_MAX = np.iinfo(np.int32).max


def popcount_rows(x):
    """uint8 [..., nb] -> int32 [...]: set bits per row."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    if hasattr(np, "bitwise_count"):
        if x.shape[-1] % 8 == 0:
            return np.bitwise_count(x.view(np.uint64)).sum(axis=-1, dtype=np.int64).astype(np.int32)
        return np.bitwise_count(x).sum(axis=-1, dtype=np.int64).astype(np.int32)
    return _POP8[x].sum(axis=-1, dtype=np.int64).astype(np.int32)


def hamming_distances(gallery, query, block=65536):
    """gallery uint8 [N, nb], query uint8 [nb] -> int32 [N]."""
    gallery = np.asarray(gallery, np.uint8)
    out = np.empty(gallery.shape[0], np.int32)
    for r in range(0, gallery.shape[0], block):
        out[r:r + block] = popcount_rows(gallery[r:r + block] ^ query[None, :])
    return out


def hamming_truth(gallery, queries, k, row_offset=0, allowed=None):
    """-> (ids int64 [Q,k], dist int32 [Q,k]) by (distance asc, id asc) over the rows `allowed` (bool [N]) admits; padded with
    -1 / INT32_MAX.  Also returns the full distance rows as a third value, int32 [Q, N]."""
    gallery, queries = np.asarray(gallery, np.uint8), np.asarray(queries, np.uint8)
    n, nq = gallery.shape[0], queries.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), INT32_MAX, np.int32)
    full = np.empty((nq, n), np.int32)
    rows = np.arange(n, dtype=np.int64) if allowed is None else np.flatnonzero(np.asarray(allowed, bool)).astype(np.int64)
    for i in range(nq):
        d = hamming_distances(gallery, queries[i]) if n else np.empty(0, np.int32)
        full[i] = d
        order = np.lexsort((rows, d[rows]))[:k]
        ids[i, :order.size] = rows[order] + int(row_offset)
        dist[i, :order.size] = d[rows][order]
    return ids, dist, full


def greedyhash_restated(K, train01, test01):
    """matching_Greedyhash (src/utils/nnsearch.py:1001-1013) with a stable order: (distance, id)."""
    train01, test01 = np.asarray(train01).astype(np.int64), np.asarray(test01).astype(np.int64)
    idx = np.zeros((test01.shape[0], K), dtype=np.int64)
    for row in range(test01.shape[0]):
        dist = (test01[row, :] ^ train01).sum(axis=1)
        idx[row, :] = np.lexsort((np.arange(train01.shape[0]), dist))[:K]
    return idx


def tie_aware_equal(idx_ref, idx_ours, train01, test01):
    """The comparison against the reference's unstable argsort: at every position the distance of the reference's id equals
    the distance of ours, and per query the sets of ids strictly below the K-th distance are equal.  -> list of complaints."""
    train01, test01 = np.asarray(train01).astype(np.int64), np.asarray(test01).astype(np.int64)
    bad = []
    for row in range(test01.shape[0]):
        dist = (test01[row, :] ^ train01).sum(axis=1)
        dr, do = dist[idx_ref[row]], dist[idx_ours[row]]
        if not np.array_equal(dr, do):
            bad.append("query %d: distances differ %s vs %s" % (row, dr.tolist(), do.tolist()))
            continue
        kth = do[-1]
        if set(idx_ref[row][dr < kth].tolist()) != set(idx_ours[row][do < kth].tolist()):
            bad.append("query %d: ids below the K-th distance differ" % row)
    return bad
