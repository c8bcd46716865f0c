"""Plain numpy / heapq restatement of the graph index (mi_graph_search, mi_graph_build), the case sweep of
tests/test_gpu_graph.py and its seeded inputs.  The truth computes no value itself: it takes a full value matrix [Q, n] from
entry points that exist without the graph index (value_matrix below: mi_refine with every id as candidate, checked against
mi_knn_dense64_search_l2 on an L2 gallery), so value ties are tested exactly, not avoided."""
import heapq

import numpy as np

NS = [1, 2, 65, 300, 3000]
DS = [1, 5, 257, 2048]
RS = [2, 4, 32, 64]
EFS = [1, 2, 8, 64, 65, 2048]
KMODES = ["one", "ef"]
NQS = [1, 5, 130]
NES = [1, 3, 64]


def search_truth(values, table, entries, k, ef, l2, row_offset=0):
    """values float64 [Q, n] (distances if l2, else inner products), table int [n, R], entries int [ne] ->
    (ids int64 [Q, k], val float64 [Q, k], visited int32 [Q]).  The ORDER is (value best first, id ascending)."""
    values = np.asarray(values, np.float64)
    table = np.asarray(table)
    nq, n = values.shape
    ids = np.full((nq, k), -1, np.int64)
    val = np.full((nq, k), np.inf if l2 else -np.inf, np.float64)
    nvis = np.zeros(nq, np.int32)
    for q in range(nq):
        key = (values[q] if l2 else 0.0 - values[q]).tolist()
        visited, expanded, first = set(), set(), []
        for e in (int(x) for x in entries):
            if e not in visited:
                visited.add(e)
                first.append((key[e], e))
        W = heapq.nsmallest(ef, first)                       # sorted by (key, id)
        for _ in range(n):                                   # (every expansion marks a row that was not expanded before)
            row = next((r for _, r in W if r not in expanded), None)
            if row is None:
                break
            expanded.add(row)
            new = []
            for c in (int(x) for x in table[row]):
                if c < 0 or c >= n or c in visited:
                    continue
                visited.add(c)
                new.append((key[c], c))
            if new:
                W = list(heapq.merge(W, sorted(new)))[:ef]
        else:
            assert all(r in expanded for _, r in W)
        nvis[q] = len(visited)
        for j, (_, r) in enumerate(W[:k]):
            ids[q, j] = row_offset + r
            val[q, j] = values[q, r]
    return ids, val, nvis


def build_truth(values, R, ne, l2):
    """values float64 [n, n], row i the values of stored row i as a query -> (table int32 [n, R], entries int32 [min(ne, n)]) as
    mi_graph_build defines them."""
    values = np.asarray(values, np.float64)
    n = values.shape[0]
    ks, h = min(R + 1, n), R // 2
    rows = np.arange(n)
    F = []
    for i in range(n):
        order = np.lexsort((rows, values[i] if l2 else 0.0 - values[i]))[:ks].tolist()
        lst = [j for j in order if j != i]
        if len(lst) == ks:
            lst = lst[:-1]
        F.append(lst)
    B = [[] for _ in range(n)]
    for j in range(n):
        for p, i in enumerate(F[j][:h]):
            B[i].append((p, j))
    table = np.full((n, R), -1, np.int32)
    for i in range(n):
        out = list(F[i][:h])
        took = 0
        for _, j in sorted(B[i]):
            if took == h or len(out) == R:
                break
            if j not in out:
                out.append(j)
                took += 1
        for j in F[i][h:]:
            if len(out) == R:
                break
            if j not in out:
                out.append(j)
        table[i, :len(out)] = out
    nent = min(ne, n)
    return table, np.array([t * n // nent for t in range(nent)], np.int32)


def value_matrix(gallery, q, l2):
    """float64 [Q, n]: the library's own value of every (query, row) pair from code the graph index does not touch: mi_refine with
    every id as candidate (kc = n <= 4096), under both metrics.  On an L2 gallery these are the bits of mi_knn_search_l2, which is
    what the contract names; mi_knn_dense64_search_l2 with k = n, the independent checker, sums the same squares in another order
    (one thread per pair, not one wave), so it agrees to rounding, not to the bit, and serves here as a second opinion within the
    bound (d + 4) 2^-53 (||q||^2 + ||g||^2) of DESIGN.md 5.11 on each side."""
    n, off = gallery.n, gallery.row_offset
    assert n <= 4096
    q = np.ascontiguousarray(q, np.float32)
    out = np.empty((q.shape[0], n), np.float64)
    cand = np.broadcast_to(np.arange(off, off + n, dtype=np.int64), (q.shape[0], n))
    ids, _, v64, _ = gallery.refine(q, cand, n)
    assert (np.sort(ids, axis=1) == np.arange(off, off + n)).all()
    np.put_along_axis(out, ids - off, v64, axis=1)
    if l2:
        ids2, _, d64, _ = gallery.dense64_search_l2(q, n)
        dense = np.empty_like(out)
        np.put_along_axis(dense, ids2 - off, d64, axis=1)
        rows = gallery_rows(gallery)
        bound = (q.shape[1] + 4) * 2.0 ** -53 * ((q.astype(np.float64) ** 2).sum(1)[:, None] + (rows.astype(np.float64) ** 2).sum(1)[None, :])
        assert (np.abs(dense - out) <= 2 * bound).all()
    return out


def gallery_rows(gallery):
    """The stored rows of a gallery, float32 [n, d] (mi_gallery_get_rows)."""
    import ctypes as C
    from isehr_amd import _lib
    rows = np.empty((gallery.n, gallery.d), np.float32)
    _lib.check(_lib.load().mi_gallery_get_rows(gallery._h, 0, gallery.n, C.c_void_p(rows.ctypes.data)))
    return rows


def sweep_cases():
    """40 cases (n, d, R, ef, kmode, nq, ne, l2, row_offset) touching every value of every axis under both metrics and both kinds
    of offset; the number of queries drops where the host truth would take more than a moment."""
    cases = []
    for i in range(40):
        n = NS[i % 5]
        d = DS[(i + i // 5) % 4]
        R = RS[(i + i // 4) % 4]
        ef = EFS[(i + i // 6) % 6]
        nq = NQS[(i + i // 3) % 3]
        ne = NES[(i + i // 9) % 3]
        while nq > 1 and nq * n * min(ef, n) > 3e6:
            nq = NQS[NQS.index(nq) - 1]
        cases.append((n, d, R, ef, KMODES[(i + i // 2) % 2], nq, ne, i % 2 == 0, 0 if (i // 2) % 2 == 0 else 1000003))
    return cases


def k_of(ef, kmode):
    return 1 if kmode == "one" else ef


def random_table(rng, n, R):
    """Seeded table with -1 padding anywhere in a row, self-loops and repeats."""
    t = rng.integers(0, n, size=(n, R)).astype(np.int32)
    t[rng.random((n, R)) < 0.2] = -1
    loops = rng.random(n) < 0.3
    t[loops, 0] = np.flatnonzero(loops)
    if R >= 2:
        t[:, R - 1] = np.where(rng.random(n) < 0.3, t[:, 0], t[:, R - 1])
    return t


def case_inputs(case):
    """-> (rows f32 [n, d], q f32 [nq, d], table int32 [n, R], entries int32 [ne]), all seeded; entries repeat once ne > n."""
    n, d, R, ef, _, nq, ne, _, _ = case
    rng = np.random.default_rng(hash((n, d, R, ef, nq, ne)) % (2 ** 31))
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return rows, q, random_table(rng, n, R), rng.integers(0, n, size=ne).astype(np.int32)
