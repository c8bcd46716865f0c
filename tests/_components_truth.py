"""Plain host truth of the connected components (mi_components): a union-find over a Python list in which the
smaller root wins, so the label of a component is its smallest row.  Written without a look at the kernel: sequential, one edge
at a time, path halving in find."""
import numpy as np


def components_truth(n, i, j):
    """n rows, edges (i[e], j[e]) -> (labels int32 [n]: the smallest row of every row's component, n_groups)"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    labels = np.array([find(v) for v in range(n)], dtype=np.int32).reshape(n)
    return labels, int((labels == np.arange(n)).sum())


def csr_pairs(row0, lims, idx):
    """the CSR output of a self-join (query q is row row0 + q) -> (i, j) int64"""
    lims = np.asarray(lims, dtype=np.int64)
    return np.repeat(np.arange(row0, row0 + lims.size - 1, dtype=np.int64), np.diff(lims)), np.asarray(idx, dtype=np.int64)
