"""Pure-numpy truth of the IVF index over PQ codes (tests only), on top of _pq_truth: a query's probes are the lists smallest by
(float64 distance to the coarse centroid, list id); its answer is pq_truth over the rows whose list is in its probe set."""
import numpy as np

from _pq_truth import adc_truth, dtable64


def probe_truth(x, G, nprobe):
    """x [Q, d], G [nlist, d] float32 -> int32 [Q, nprobe]: a lexsort of (dtable64(x, G[None])[0], list id)."""
    G = np.asarray(G, np.float32)
    acc = dtable64(x, G[None])[0][:, 0, :]                               # [Q, nlist] float64, before any rounding
    ids = np.arange(G.shape[0])
    return np.stack([np.lexsort((ids, acc[i]))[:nprobe] for i in range(acc.shape[0])]).astype(np.int32)


def ivfpq_truth(x, C, codes, lists, probes, k, row_offset=0, allowed=None):
    """probes integer [Q, P] (-1 = no list, repeats allowed) -> (ids int64 [Q, k], dist float32 [Q, k]): what pq_truth gives
    query by query with allowed & isin(lists, probe set) -- the distances of pq_truth (computed once for the batch), the rows a
    query admits, order by (distance asc, id asc), padding -1 / +inf."""
    lists = np.asarray(lists)
    probes = np.asarray(probes)
    base = np.ones(lists.shape[0], bool) if allowed is None else np.asarray(allowed, bool)
    dist_all = adc_truth(dtable64(x, C)[1], codes)
    nq = dist_all.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float32)
    for i in range(nq):
        rows = np.flatnonzero(base & np.isin(lists, probes[i][probes[i] >= 0])).astype(np.int64)
        d = dist_all[i, rows]
        order = np.lexsort((rows, d))[:k]
        ids[i, :order.size] = rows[order] + int(row_offset)
        dist[i, :order.size] = d[order]
    return ids, dist
