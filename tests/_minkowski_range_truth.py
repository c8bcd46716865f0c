"""numpy truth of the Minkowski radius search (csrc/minkowski_range.hip): the CSR contract restated on the values of
tests/_minkowski_truth.py, no device, no library.

A hit of query i is an admitted row with value <= radius in float64 (inclusive; a NaN never is one); the hits of a query are ordered
by (value asc, id asc), ids are row_offset + local row, and lims is the running count of hits: the hits of query i are
ids / dist64[lims[i]:lims[i + 1]].  The self-join reports, for the query that is stored row r, only the rows above r."""
import numpy as np

from _minkowski_truth import values  # noqa: F401  (re-exported: the value of every pair is the top-K search's)


def threshold(vals, radius, allow=None, above=None):
    """vals float64 [nq, n] -> bool [nq, n]: value <= radius among the rows `allow` (None or a bool mask [n]) admits; above: None or
    int [nq], query i keeps only the rows > above[i] (the self-join)."""
    vals = np.asarray(vals, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        hit = vals <= float(radius)                                        # (a NaN compares false)
    if allow is not None:
        hit &= np.asarray(allow, dtype=np.bool_)[None, :]
    if above is not None:
        hit &= np.arange(vals.shape[1])[None, :] > np.asarray(above, dtype=np.int64)[:, None]
    return hit


def csr(vals, radius, allow=None, row_offset=0, above=None):
    """-> (lims int64 [nq + 1], ids int64 [lims[-1]], dist64 float64 [lims[-1]]): per query a stable sort by value of the hits in
    ascending row order, which is the order (value asc, id asc)."""
    vals = np.asarray(vals, dtype=np.float64)
    hit = threshold(vals, radius, allow, above)
    lims = np.zeros(vals.shape[0] + 1, dtype=np.int64)
    ids, dist = [], []
    for i in range(vals.shape[0]):
        rows = np.flatnonzero(hit[i])
        order = rows[np.argsort(vals[i, rows], kind="stable")]
        ids.append(order + row_offset)
        dist.append(vals[i, order])
        lims[i + 1] = lims[i] + order.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return lims, cat(ids, np.int64), cat(dist, np.float64)


def pairs(vals, radius):
    """The self-join of a whole gallery: vals float64 [n, n] -> (pairs int64 [P, 2] with i < j, dist64 [P]) in the order of i, then
    of (value asc, j asc)."""
    n = vals.shape[0]
    lims, ids, dist = csr(vals, radius, above=np.arange(n))
    return np.stack([np.repeat(np.arange(n, dtype=np.int64), np.diff(lims)), ids], axis=1), dist
