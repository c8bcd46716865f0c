"""Plain-Python truth of the grouped top-K search (mi_knn_search_grouped) and the two sources of the complete
ranking it walks.

grouped_truth is the contract restated as a loop: walk a query's complete ranking, (score desc, id asc), from the top; keep a row
if its group has not been kept yet and its label is not the query's excluded label; stop at k kept rows; pad with -1 / -inf / -1.

The ranking comes from
  (a) library_ranking   the library's own full ranking from code that exists without the grouped search: Gallery.search(q, n) for
                        n <= 2048, whose scores are search's own bits on ANY data, and Gallery.rank_all above.  rank_all orders by
                        the float32 FMA scores of the f32 scorer, which are search's bits only where every score is exact, so the
                        tests use it on lattice data alone;
  (b) lattice_ranking   tests/_lattice_truth.py's integer lattice, every product and sum exact: numpy int64 scores ordered by
                        np.lexsort((ids, -scores)), which no summation order can change.
"""
import numpy as np

import _lattice_truth as lt


def grouped_truth(order_ids, order_scores, labels, k, exclude=None, row_offset=0):
    """order_ids int64 [nq, m] (global ids: row_offset + local row) and order_scores float32 [nq, m]: every query's COMPLETE ranking;
    labels [n] (>= 0 a group, -1 a group of its own); exclude None or one label per query (-1, or a label no row has: nothing)
    -> ids int64 [nq, k], scores float32 [nq, k], labels int32 [nq, k]"""
    order_ids, order_scores = np.asarray(order_ids), np.asarray(order_scores, dtype=np.float32)
    labels = [int(v) for v in np.asarray(labels)]
    nq = order_ids.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    scores = np.full((nq, k), -np.inf, np.float32)
    labs = np.full((nq, k), -1, np.int32)
    for q in range(nq):
        ex = -1 if exclude is None else int(exclude[q])
        seen, kept = set(), 0
        row_ids = order_ids[q].tolist()
        for j, gid in enumerate(row_ids):
            if kept == k:
                break
            lab = labels[gid - row_offset]
            group = lab if lab >= 0 else ("row", gid)
            if group in seen or (ex >= 0 and lab == ex):
                continue
            seen.add(group)
            ids[q, kept], scores[q, kept], labs[q, kept] = gid, order_scores[q, j], lab
            kept += 1
    return ids, scores, labs


def library_ranking(g, Q):
    """(a): -> ids int64 [nq, n], scores float32 [nq, n] from Gallery.search (n <= 2048) or Gallery.rank_all"""
    if g.n <= 2048:
        ids, sc, _ = g.search(Q, g.n)
    else:
        ids, sc, _ = g.rank_all(Q, return_scores=True)
    return ids, sc


def lattice_ranking(X, Q, row_offset=0):
    """(b): integer-lattice rows X [n, d] and queries Q [nq, d] -> ids int64 [nq, n], scores float32 [nq, n]"""
    S = lt.int_scores(X, Q)
    rows = np.arange(S.shape[1], dtype=np.int64)
    order = np.stack([np.lexsort((rows, -s)) for s in S])
    return order + row_offset, np.take_along_axis(S, order, axis=1).astype(np.float32)


def random_labels(rng, n, max_size=7, singles=0.2, spread=1):
    """labels int32 [n]: groups of 1 .. max_size rows scattered over the gallery, labels `spread` apart (not dense), a share
    `singles` of the rows labelled -1"""
    labels = np.empty(n, np.int64)
    i, lab = 0, 0
    while i < n:
        size = int(rng.integers(1, max_size + 1))
        labels[i:i + size] = lab * spread
        i, lab = i + size, lab + 1
    labels = rng.permutation(labels)
    labels[rng.random(n) < singles] = -1
    return labels.astype(np.int32)


def reference_negatives(ranks, pool_clusters, query_clusters, nnum):
    """The selection loop of the reference's create_epoch_tuples (src/datasets/traindataset.py:226-243) on ranks [P, Q] (column q: the
    pool positions of query q, best first) -> nidxs int64 [Q, nnum].  Where the reference would run off the end of the column
    (IndexError) the rest of the row is -1."""
    P, Q = ranks.shape
    out = np.full((Q, nnum), -1, np.int64)
    for q in range(Q):
        clusters = [int(query_clusters[q])]
        nidxs = []
        r = 0
        while len(nidxs) < nnum and r < P:
            potential = int(ranks[r, q])
            if not int(pool_clusters[potential]) in clusters:
                nidxs.append(potential)
                clusters.append(int(pool_clusters[potential]))
            r += 1
        out[q, :len(nidxs)] = nidxs
    return out
