"""The IVF-Flat index (mi_ivfflat*) restated in numpy: float64 values, the order (value best first, id ascending),
probes, assignment, list layout, normalisation of a caller's probes, the answer with its padding and the count of rows evaluated.
On lattice data (integer-valued float32 in [-3, 3]) every float64 sum is exact in any order, so these are the library's bits."""
import numpy as np


def lattice(rng, shape):
    """Integer-valued float32 in [-3, 3]: large tie classes, sums exact in float64 whatever their order."""
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def values(q, rows, l2):
    """float64 [Q, N]: squared distances in the direct form (L2), inner products otherwise, from the float32 values promoted."""
    q, rows = np.asarray(q, np.float32).astype(np.float64), np.asarray(rows, np.float32).astype(np.float64)
    if not l2:
        return q @ rows.T
    out = np.zeros((len(q), len(rows)))
    for j in range(q.shape[1]):                                 # (column by column: no [Q, N, d] array)
        out += (q[:, j, None] - rows[None, :, j]) ** 2
    return out


def order(vals, ids, l2):
    """Positions of `vals` sorted by (value best first, id ascending)."""
    return np.lexsort((ids, vals if l2 else -vals))


def probe(q, centroids, nprobe, l2):
    """int32 [Q, nprobe]: the nprobe best lists of every query in the order."""
    v = values(q, centroids, l2)
    lists = np.arange(v.shape[1])
    return np.stack([lists[order(v[i], lists, l2)][:nprobe] for i in range(v.shape[0])]).astype(np.int32).reshape(len(v), nprobe)


def assign(stored, centroids, l2):
    """int32 [N]: the probe-1 list of every stored row."""
    stored = np.asarray(stored)
    return np.concatenate([probe(stored[i:i + 1024], centroids, 1, l2)[:, 0] for i in range(0, len(stored), 1024)])


def lists_of(list_ids, nlist):
    """(list_off int64 [nlist + 1], list_rows int32 [n]): rows ascending within a list."""
    list_ids = np.asarray(list_ids)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(list_ids, minlength=nlist))
    return off, np.argsort(list_ids, kind="stable").astype(np.int32)


def normalise(probes, nlist):
    """A caller's probe rows: an entry outside [0, nlist) or repeating an earlier entry of its row becomes -1."""
    out = np.asarray(probes).astype(np.int64).copy()
    for row in out:
        seen = set()
        for i, v in enumerate(row):
            if v < 0 or v >= nlist or int(v) in seen:
                row[i] = -1
            else:
                seen.add(int(v))
    return out.astype(np.int32)


def candidates(probes, list_off, list_rows, nlist, allow=None):
    """Per query the local rows of its (normalised) probed lists that the bool mask `allow` admits, as one int64 array each."""
    out = []
    for row in normalise(probes, nlist):
        c = [list_rows[list_off[l]:list_off[l + 1]] for l in row if l >= 0]
        c = np.concatenate(c).astype(np.int64) if c else np.zeros(0, np.int64)
        out.append(c if allow is None else c[np.asarray(allow)[c]])
    return out


def search(q, stored, probes, list_off, list_rows, nlist, k, l2, row_offset=0, allow=None):
    """-> (ids int64 [Q, k], values float64 [Q, k], scanned int64 [Q])."""
    q = np.asarray(q, np.float32)
    cand = candidates(probes, list_off, list_rows, nlist, allow)
    ids = np.full((len(q), k), -1, np.int64)
    vals = np.full((len(q), k), np.inf if l2 else -np.inf)
    for i, c in enumerate(cand):
        v = values(q[i:i + 1], stored[c], l2)[0]
        o = order(v, c, l2)[:k]
        ids[i, :len(o)] = c[o] + row_offset
        vals[i, :len(o)] = v[o]
    return ids, vals, np.array([len(c) for c in cand], np.int64)
