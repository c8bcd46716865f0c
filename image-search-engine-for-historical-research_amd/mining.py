"""Hard-negative mining on the device: the selection loop of the reference's create_epoch_tuples
(src/datasets/traindataset.py:219-243 and :466-490) as one grouped top-K search.

The reference scores the whole negative pool against every query with torch.mm, sorts every column in full, walks it from the top,
skips the query's own cluster and takes at most one image per cluster until it has `nnum`.  That is Gallery.search_grouped with the
clusters as groups and the query's cluster excluded: raw inner products (a NORM_NONE gallery), ties to the lower pool position.
"""
import numpy as np

from ._lib import Gallery, NORM_NONE, group_labels


def hard_negatives_hip(qvecs, poolvecs, pool_clusters, query_clusters, nnum, device=0):
    """qvecs [D, Q] and poolvecs [D, P] in the reference's layout (numpy or CPU torch, float32 / float64), pool_clusters [P] and
    query_clusters [Q] integer cluster ids >= 0 -> (nidxs int64 [Q, nnum], avg_ndist float).

    nidxs[q] holds POOL POSITIONS, best first: the caller maps them through its idxs2images.  avg_ndist is the reference's
    statistic, the mean of sqrt(sum((q - p + 1e-6) ** 2)) over the chosen pairs, computed here in float64 on the host from the
    chosen columns (the reference accumulates it in float32 on the device).

    Where the reference differs: it raises an IndexError when a query runs out of clusters before it has nnum negatives
    (`ranks[r, q]` past the pool); here the rest of that row is -1 and the pairs that exist enter the statistic (nan if there is
    none at all)."""
    qv = qvecs.numpy() if hasattr(qvecs, "numpy") and not isinstance(qvecs, np.ndarray) else np.asarray(qvecs)
    pv = poolvecs.numpy() if hasattr(poolvecs, "numpy") and not isinstance(poolvecs, np.ndarray) else np.asarray(poolvecs)
    if qv.ndim != 2 or pv.ndim != 2 or qv.shape[0] != pv.shape[0]:
        raise ValueError("qvecs [D, Q] and poolvecs [D, P] must share D")
    pool_clusters, query_clusters = group_labels(pool_clusters), group_labels(query_clusters)
    if pool_clusters.size != pv.shape[1] or query_clusters.size != qv.shape[1]:
        raise ValueError("one cluster id per pool column and per query column")
    if (pool_clusters.size and pool_clusters.min() < 0) or (query_clusters.size and query_clusters.min() < 0):
        raise ValueError("cluster ids must be >= 0")
    nnum = int(nnum)
    with Gallery.from_host(pv.T, norm_mode=NORM_NONE, device=device) as g:
        g.set_groups(pool_clusters)
        nidxs = g.search_grouped(qv.T, nnum, exclude=query_clusters)[0]
    q_of, slot = np.nonzero(nidxs >= 0)
    diff = qv[:, q_of].astype(np.float64) - pv[:, nidxs[q_of, slot]].astype(np.float64) + 1e-6
    dist = np.sqrt((diff * diff).sum(axis=0))
    return nidxs, float(dist.mean()) if dist.size else float("nan")
