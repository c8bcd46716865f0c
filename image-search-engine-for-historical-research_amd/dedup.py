"""Near-duplicate pairs of a gallery: every pair of stored rows i < j whose exact score is >= min_score.

The same print, photo or scan often enters an archive database more than once when several archives are merged
(the reference's `src/offline.py --datasets 'A, B, ...'`); this finds those copies as a self-join of exact range searches
(Gallery.range_search) with the gallery's own stored rows as queries.  near_duplicate_pairs_hamming is the same
join on the hash codes of a binary index (BinaryGallery.self_range): integer distances, 256 bytes per row at 2048
bits instead of 8 KiB, and the queries never leave the device.  near_duplicate_pairs_minkowski is the join on the raw rows in
L1, L-infinity, Lp or squared L2 (Gallery.self_range_minkowski): exact float64 values, the queries read on the device.

near_duplicate_groups* are the same three joins closed transitively ("a ~ b and b ~ c: one item") by a union-find on the device
(_lib.Components): one int32 label per row, the smallest row of its group, ready for Gallery.set_groups.  The
Hamming form never makes a pair: the union reads the 64-bit ballots of the self-join's scan.
"""
import numpy as np

from . import _lib


def near_duplicate_pairs(gallery, min_score, batch=1024):
    """-> (i int64, j int64, score float32): all pairs i < j with exact score >= min_score (inclusive), in the order of
    i, then of (score desc, j asc).  Stored row i is the query of its pairs: each pair is reported once, with the score of
    the range search of row i, and self pairs drop out.  Assumes a single-shard gallery with row_offset 0 (ids are rows)."""
    if gallery.row_offset != 0:
        raise ValueError("near_duplicate_pairs needs a gallery with row_offset 0 (a single shard)")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    out_i, out_j, out_s = [], [], []
    for r0 in range(0, gallery.n, batch):
        m = min(batch, gallery.n - r0)
        rows = gallery.get_rows(r0, m)
        lims, idx, sc, _ = gallery.range_search(rows, min_score)
        qi = np.repeat(np.arange(r0, r0 + m, dtype=np.int64), np.diff(lims))
        keep = idx > qi
        out_i.append(qi[keep])
        out_j.append(np.asarray(idx, dtype=np.int64)[keep])
        out_s.append(np.asarray(sc, dtype=np.float32)[keep])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_s)


def near_duplicate_pairs_hamming(binary, radius, batch=1024):
    """-> (i int64, j int64, dist int32): all pairs of stored codes i < j with Hamming distance <= radius (inclusive), in the
    order of i, then of (distance asc, j asc).  `binary` is a BinaryGallery or an LSHIndex (its gallery is joined).  The join
    runs as self_range calls over `batch` rows at a time, so the memory in flight is that of one batch's pairs.  Assumes a
    single-shard index with row_offset 0 (ids are rows)."""
    g = getattr(binary, "gallery", binary)
    if g.row_offset != 0:
        raise ValueError("near_duplicate_pairs_hamming needs an index with row_offset 0 (a single shard)")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    out_i, out_j, out_d = [], [], []
    for r0 in range(0, g.n, batch):
        m = min(batch, g.n - r0)
        lims, idx, dist, _ = g.self_range(r0, m, radius)
        out_i.append(np.repeat(np.arange(r0, r0 + m, dtype=np.int64), np.diff(lims)))
        out_j.append(np.asarray(idx, dtype=np.int64))
        out_d.append(np.asarray(dist, dtype=np.int32))
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)


def near_duplicate_pairs_minkowski(gallery, radius, metric="lp", p=2, batch=1024):
    """-> (pairs int64 [P, 2] with i < j, dist64 float64 [P]): all pairs of stored rows whose Minkowski value is <= radius
    (inclusive), in the order of i, then of (value asc, j asc).  metric "l1", "linf" or "lp" with p > 0 (the default, p = 2, is the
    squared Euclidean distance; the radius applies to sum |x_i - x_j| ** p, not to its 1 / p-th power).  The join runs as
    self_range_minkowski calls over `batch` rows at a time.  Assumes a single-shard gallery with row_offset 0 (ids are rows)."""
    if gallery.row_offset != 0:
        raise ValueError("near_duplicate_pairs_minkowski needs a gallery with row_offset 0 (a single shard)")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    out_i, out_j, out_d = [], [], []
    for r0 in range(0, gallery.n, batch):
        m = min(batch, gallery.n - r0)
        lims, idx, _, dist64, _ = gallery.self_range_minkowski(r0, m, radius, metric, p)
        out_i.append(np.repeat(np.arange(r0, r0 + m, dtype=np.int64), np.diff(lims)))
        out_j.append(np.asarray(idx, dtype=np.int64))
        out_d.append(np.asarray(dist64, dtype=np.float64))
    if not out_i:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.float64)
    return np.stack([np.concatenate(out_i), np.concatenate(out_j)], axis=1), np.concatenate(out_d)


def _groups(n, device, batch, add):
    """The join loop of the three functions below: add(cc, r0, m) hands the hits of stored rows [r0, r0 + m) to the union-find."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    with _lib.Components(n, device) as cc:
        for r0 in range(0, n, batch):
            add(cc, r0, min(batch, n - r0))
        return cc.labels()


def near_duplicate_groups(gallery, min_score, batch=1024):
    """-> (labels int32 [n], n_groups): rows i, j are in one group when a chain of pairs with exact score >= min_score joins
    them (the pairs of near_duplicate_pairs, closed transitively); labels[v] is the smallest row of v's group, so
    gallery.set_groups(labels) collapses near duplicates in search_grouped.  Each batch's range-search CSR goes to the device
    union-find; nothing is concatenated.  Assumes a single-shard gallery with row_offset 0 (ids are rows)."""
    if gallery.row_offset != 0:
        raise ValueError("near_duplicate_groups needs a gallery with row_offset 0 (a single shard)")

    def add(cc, r0, m):
        lims, idx, _, _ = gallery.range_search(gallery.get_rows(r0, m), min_score)
        cc.add_csr(r0, lims, idx)
    return _groups(gallery.n, gallery.device, batch, add)


def near_duplicate_groups_minkowski(gallery, radius, metric="lp", p=2, batch=1024):
    """-> (labels int32 [n], n_groups): the groups of the pairs of near_duplicate_pairs_minkowski (Minkowski value <= radius,
    metric and p as there), closed transitively.  Assumes a single-shard gallery with row_offset 0 (ids are rows)."""
    if gallery.row_offset != 0:
        raise ValueError("near_duplicate_groups_minkowski needs a gallery with row_offset 0 (a single shard)")

    def add(cc, r0, m):
        lims, idx, _, _, _ = gallery.self_range_minkowski(r0, m, radius, metric, p)
        cc.add_csr(r0, lims, idx)
    return _groups(gallery.n, gallery.device, batch, add)


def near_duplicate_groups_hamming(binary, radius, batch=1024):
    """-> (labels int32 [n], n_groups): the groups of the pairs of near_duplicate_pairs_hamming (Hamming distance <= radius),
    closed transitively.  `binary` is a BinaryGallery or an LSHIndex (its gallery is joined).  No pair ever reaches the host, or
    exists on the device: each batch of `batch` stored rows is scanned and united from the scan's ballots
    (Components.add_hamming_self).  Assumes a single-shard index with row_offset 0 (ids are rows)."""
    g = getattr(binary, "gallery", binary)
    if g.row_offset != 0:
        raise ValueError("near_duplicate_groups_hamming needs an index with row_offset 0 (a single shard)")
    return _groups(g.n, g.device, batch, lambda cc, r0, m: cc.add_hamming_self(g, r0, m, radius))
