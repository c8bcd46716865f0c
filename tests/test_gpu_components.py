"""GPU: connected components on the device (mi_components, csrc/components.hip, csrc/api_components.hip)
against the host union-find of tests/_components_truth.py.  Everything is integer and exact: labels and group counts are compared
with array_equal, whatever the source of the edges (pair lists, self-join CSR, the Hamming self-join's ballots), their order,
their split into calls and the memory they live in."""
import numpy as np
import pytest

import _grouped_truth as gt
import _lattice_truth as lt
import _minkowski_range_truth as MR
import _minkowski_truth as MT
from _components_truth import components_truth, csr_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def _add(cc, i, j, device):
    if device:
        ti, tj = _dev(i), _dev(j)
        cc.add_pairs_device(ti.data_ptr(), tj.data_ptr(), ti.numel())
    else:
        cc.add_pairs(i, j)


def _labels(cc, device):
    if not device:
        return cc.labels()
    import torch
    out = torch.full((max(cc.n, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    groups = cc.labels_device(out.data_ptr())
    return out.cpu().numpy()[:cc.n], groups


def _check_pairs(lib, n, i, j, device, want=None):
    want = components_truth(n, i, j) if want is None else want
    with lib.Components(n) as cc:
        assert cc.n == n
        _add(cc, i, j, device)
        labels, groups = _labels(cc, device)
    assert labels.dtype == np.int32 and labels.shape == (n,)
    assert np.array_equal(labels, want[0]), np.flatnonzero(labels != want[0])[:8]
    assert groups == want[1]
    return labels


# ---- 1. pairs against the truth
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_random_pairs(lib, n, device):
    rng = np.random.default_rng(7 * n + device)
    for m in sorted({0, 1, n // 2, 4 * n}):
        i, j = rng.integers(0, n, m), rng.integers(0, n, m)
        _check_pairs(lib, n, i, j, device)


@pytest.fixture(scope="module")
def path_edges():
    a = np.arange(65535, dtype=np.int64)
    return {"ascending": (a, a + 1), "descending": (a[::-1] + 1, a[::-1]), "shuffled": (np.random.default_rng(3).permutation(a), None)}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_path_graph_is_one_component(lib, path_edges, order, device):
    """the deep tree of find and flatten: 65 536 rows in one chain"""
    n = 65536
    i, j = path_edges[order]
    if j is None:
        j = i + 1
    labels = _check_pairs(lib, n, i, j, device, want=(np.zeros(n, np.int32), 1))
    assert (labels == 0).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_star_contention_and_late_join(lib, device):
    n = 4096                                                   # a star with its hub at the largest id
    _check_pairs(lib, n, np.full(n - 1, n - 1), np.arange(n - 1), device, want=(np.zeros(n, np.int32), 1))
    edges = np.array([[5, 900], [900, 17], [3, 4]])            # 200 000 copies of three distinct edges: one root under fire
    pick = np.random.default_rng(11).integers(0, 3, 200_000)
    want = np.arange(1000, dtype=np.int32)
    want[[17, 900]] = 5
    want[4] = 3
    _check_pairs(lib, 1000, edges[pick, 0], edges[pick, 1], device, want=(want, 997))
    a = np.arange(1999)                                        # two components of 2 000 rows, joined by the very last edge
    i, j = np.concatenate([a, a + 2000]), np.concatenate([a + 1, a + 2001])
    _check_pairs(lib, 4000, i, j, device, want=(np.repeat(np.array([0, 2000], np.int32), 2000), 2))
    _check_pairs(lib, 4000, np.append(i, 3999), np.append(j, 1999), device, want=(np.zeros(4000, np.int32), 1))
    loops = np.random.default_rng(12).integers(0, 777, 3000)   # i == j edges only
    _check_pairs(lib, 777, loops, loops, device, want=(np.arange(777, dtype=np.int32), 777))


# ---- 2. order and split independence
def test_order_and_split_independence(lib):
    n, m = 5000, 20000
    rng = np.random.default_rng(21)
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    want = components_truth(n, i, j)
    cuts = [0, 1, 14, 3000, 3001, 9000, 19990, m]              # 7 uneven calls
    finals = []
    with lib.Components(n) as cc:
        cc.add_pairs(i, j)
        finals.append(cc.labels())
        cc.reset()
        assert np.array_equal(cc.labels()[0], np.arange(n)) and cc.labels()[1] == n
        for a, b in zip(cuts[:-1], cuts[1:]):
            cc.add_pairs(i[a:b], j[a:b])
            part = cc.labels()                                 # labels in between: the handle goes on
            assert np.array_equal(part[0], components_truth(n, i[:b], j[:b])[0])
        finals.append(cc.labels())
        cc.reset()
        cc.add_pairs(i[::-1], j[::-1])
        finals.append(cc.labels())
        cc.reset()
        cc.add_pairs(j, i)
        finals.append(cc.labels())
        for labels, groups in finals:
            assert np.array_equal(labels, want[0]) and groups == want[1]
        # reset, then another edge list: what a fresh handle gives
        i2, j2 = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
        cc.reset()
        cc.add_pairs(i2, j2)
        again = cc.labels()
    with lib.Components(n) as fresh:
        fresh.add_pairs(i2, j2)
        new = fresh.labels()
    assert np.array_equal(again[0], new[0]) and again[1] == new[1]
    assert np.array_equal(new[0], components_truth(n, i2, j2)[0])


# ---- 3. validation
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_invalid_ids_leave_the_components_as_they_were(lib, device):
    n = 500
    rng = np.random.default_rng(31)
    i, j = rng.integers(0, n, 300), rng.integers(0, n, 300)
    with lib.Components(n) as cc:
        cc.add_pairs(i, j)
        before = cc.labels()
        for bad in (-1, n):
            for where in (0, 150, 299):
                for side in (0, 1):
                    bi, bj = i.copy(), j.copy()
                    (bi, bj)[side][where] = bad
                    with pytest.raises(RuntimeError, match="outside"):
                        _add(cc, np.append(bi, 0), np.append(bj, n - 1), device)    # the good edge (0, n - 1) must not be made
                    after = cc.labels()
                    assert np.array_equal(after[0], before[0]) and after[1] == before[1]
        lims, idx = np.array([0, 2, 3]), np.array([7, 8, 9])
        for bad_lims, bad_idx, what in ((np.array([0, 3, 2]), idx, "non-decreasing"), (np.array([1, 2, 3]), idx, "lims"),
                                        (lims, np.array([7, -1, 9]), "outside"), (lims, np.array([7, 8, n]), "outside")):
            with pytest.raises(RuntimeError, match=what):
                if device:
                    tl, ti = _dev(bad_lims), _dev(bad_idx)
                    cc.add_csr_device(3, tl.data_ptr(), ti.data_ptr(), 2)
                else:
                    cc.add_csr(3, bad_lims, bad_idx)
            assert np.array_equal(cc.labels()[0], before[0])
        with pytest.raises(RuntimeError, match="query rows"):
            cc.add_csr(n - 1, lims, idx)                       # rows n - 1 and n
        cc.add_pairs([], [])                                   # m == 0 and nq == 0 are fine
        cc.add_csr(0, [0], [])
        assert np.array_equal(cc.labels()[0], before[0])
        if device:
            tl, ti = _dev(lims), _dev(idx)
            cc.add_csr_device(3, tl.data_ptr(), ti.data_ptr(), 2)
        else:
            cc.add_csr(3, lims, idx)
        want = components_truth(n, np.concatenate([i, [3, 3, 4]]), np.concatenate([j, idx]))
        assert np.array_equal(cc.labels()[0], want[0]) and cc.labels()[1] == want[1]


# ---- 4. / 5. binary galleries with chains: a - b and b - c within the radius, a - c outside it
def _flip(code, bits):
    out = code.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


RADIUS = {64: 6, 2048: 200}                                    # random codes lie near nbits / 2: only the planted ones are this close


def _chained_codes(n, nbits):
    """random codes; 12 planted clusters at random rows: chains a - b - c (- d) whose links flip RADIUS disjoint bits each, so the
    ends are 2 (3) RADIUS apart, and exact copies"""
    rng = np.random.default_rng([n, nbits])
    r = RADIUS[nbits]
    g = rng.integers(0, 256, size=(n, nbits // 8), dtype=np.uint8)
    rows = rng.choice(n, min(n, 44), replace=False)
    k = 0
    while k + 4 <= rows.size:
        length = 3 + (k // 4) % 2
        for t in range(1, length):
            g[rows[k + t]] = _flip(g[rows[k + t - 1]], range((t - 1) * r, t * r))
        if length == 3:
            g[rows[k + 3]] = g[rows[k]]                        # an exact copy of the chain's first row
        k += 4
    return g


@pytest.fixture(scope="module", params=[(1000, 64), (1000, 2048), (130, 64)], ids=lambda p: "n%d-b%d" % p)
def binary(request, lib):
    """-> (n, nbits, index, the pairs of near_duplicate_pairs_hamming at RADIUS, their truth labels)"""
    from isehr_amd.dedup import near_duplicate_pairs_hamming
    n, nbits = request.param
    idx = lib.BinaryGallery.from_host(_chained_codes(n, nbits))
    i, j, dist = near_duplicate_pairs_hamming(idx, RADIUS[nbits])
    have = set(zip(i.tolist(), j.tolist()))
    want = components_truth(n, i, j)
    # the closure is observable: some group holds two rows that are no pair
    sizes = np.bincount(want[0], minlength=n)
    assert sizes.max() >= 4 and any((a, b) not in have for lab in np.flatnonzero(sizes >= 3)
                                    for a in np.flatnonzero(want[0] == lab) for b in np.flatnonzero(want[0] == lab) if a < b)
    yield n, nbits, idx, (i, j), want
    idx.close()


@pytest.mark.parametrize("window", [64, 100])
def test_csr_of_the_hamming_self_join(lib, binary, window):
    n, nbits, idx, _, want = binary
    with lib.Components(n) as cc:
        for r0 in range(0, n, window):
            lims, ids, _, _ = idx.self_range(r0, min(window, n - r0), RADIUS[nbits])
            cc.add_csr(r0, lims, ids)
        labels, groups = cc.labels()
    assert np.array_equal(labels, want[0]) and groups == want[1]


def test_csr_on_the_device(lib, binary):
    n, nbits, idx, _, want = binary
    lims, ids, _, _ = idx.self_range(0, n, RADIUS[nbits])
    tl, ti = _dev(lims), _dev(ids)
    with lib.Components(n) as cc:
        cc.add_csr_device(0, tl.data_ptr(), ti.data_ptr(), n)
        labels, groups = cc.labels()
    assert np.array_equal(labels, want[0]) and groups == want[1]


def _float_rows_with_copies(seed, n, d):
    """integer-lattice rows (every score and distance exact), a few of them exact copies of others, some copied twice"""
    rng = np.random.default_rng(seed)
    X = lt.int_rows(rng, n, d)
    rows = rng.choice(n, 60, replace=False)
    X[rows[20:40]] = X[rows[:20]]
    X[rows[40:50]] = X[rows[:10]]
    return X, rng


def test_csr_of_the_inner_product_join(lib):
    """Gallery.range_search with stored rows as queries; the rows list themselves among their hits, which is harmless"""
    from isehr_amd.dedup import near_duplicate_groups
    n, d = 300, 64
    X, _ = _float_rows_with_copies(41, n, d)
    S = lt.int_scores(X, X)
    tau = int(np.diag(S).min())                                # every row reaches it with itself and with its copies
    i, j = np.nonzero(np.triu(S >= tau, 1))
    want = components_truth(n, i, j)
    assert want[1] <= n - 30                                   # the 30 copied rows at the least
    with lib.Gallery.from_host(X, norm_mode=lib.NORM_NONE) as g, lib.Components(n) as cc:
        for r0 in range(0, n, 128):
            m = min(128, n - r0)
            lims, ids, _, _ = g.range_search(g.get_rows(r0, m), tau)
            cc.add_csr(r0, lims, ids)
        labels, groups = cc.labels()
        assert np.array_equal(labels, want[0]) and groups == want[1]
        for batch in (64, 1024):
            labels, groups = near_duplicate_groups(g, tau, batch=batch)
            assert labels.dtype == np.int32 and np.array_equal(labels, want[0]) and groups == want[1]


def test_csr_of_the_minkowski_join(lib):
    from isehr_amd.dedup import near_duplicate_groups_minkowski
    n, d = 300, 40
    X, _ = _float_rows_with_copies(42, n, d)
    radius = 30.0                                              # L1 on the lattice: copies at 0, unrelated rows around 90
    pairs, _ = MR.pairs(MT.values(X, X, "l1", None), radius)
    want = components_truth(n, pairs[:, 0], pairs[:, 1])
    assert want[1] <= n - 30
    with lib.Gallery.from_host(X, norm_mode=lib.NORM_NONE) as g, lib.Components(n) as cc:
        for r0 in range(0, n, 100):
            lims, ids, _, _, _ = g.self_range_minkowski(r0, min(100, n - r0), radius, "l1")
            cc.add_csr(r0, lims, ids)
        labels, groups = cc.labels()
        assert np.array_equal(labels, want[0]) and groups == want[1]
        labels, groups = near_duplicate_groups_minkowski(g, radius, "l1", batch=64)
        assert np.array_equal(labels, want[0]) and groups == want[1]


def _windows(n):
    """the windows of the issue; (37, 100) ends at the last row where the index has fewer than 137"""
    return [(0, n), (0, 64), (64, 66), (37, min(100, n - 37)), (n - 1, 1), (5, 0)]


def _ballots_against_csr(lib, idx, n, radius):
    with lib.Components(n) as a, lib.Components(n) as b:
        for row0, nrows in _windows(n):
            a.reset()
            b.reset()
            a.add_hamming_self(idx, row0, nrows, radius)
            lims, ids, _, _ = idx.self_range(row0, nrows, radius)
            b.add_csr(row0, lims, ids)
            got, want = a.labels(), b.labels()
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (row0, nrows, radius)
            if nrows == 0:
                assert got[1] == n


@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks-of-64"])
def test_ballots_against_csr(lib, binary, chunked):
    n, nbits, idx, _, want = binary
    before = [idx.self_range(0, n, RADIUS[nbits])[:3], idx.self_range(37, 64, nbits)[:3]]
    if chunked:
        lib.set_global_option("hamming_range_bytes", 1)        # the floor: 64 queries a chunk
    try:
        for radius in (0, RADIUS[nbits], nbits, nbits + 5):
            _ballots_against_csr(lib, idx, n, radius)
        with lib.Components(n) as cc:
            cc.add_hamming_self(idx, 0, n, RADIUS[nbits])      # the whole join: the truth of the pair path
            labels, groups = cc.labels()
            assert np.array_equal(labels, want[0]) and groups == want[1]
            cc.reset()
            cc.add_hamming_self(idx, 0, n, nbits)              # every pair: one component
            labels, groups = cc.labels()
            assert (labels == 0).all() and groups == 1
    finally:
        if chunked:
            lib.set_global_option("hamming_range_bytes", 0)
    assert lib.get_global_option("hamming_range_bytes") == 1 << 30
    # the index's workspace is shared with the join: the join still answers as before
    after = [idx.self_range(0, n, RADIUS[nbits])[:3], idx.self_range(37, 64, nbits)[:3]]
    for x, y in zip(before, after):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def test_groups_hamming_and_argument_errors(lib, binary):
    from isehr_amd.dedup import near_duplicate_groups_hamming
    n, nbits, idx, _, want = binary
    for batch in (64, 100, 1024):
        labels, groups = near_duplicate_groups_hamming(idx, RADIUS[nbits], batch=batch)
        assert labels.dtype == np.int32 and np.array_equal(labels, want[0]) and groups == want[1]
    with lib.Components(n + 1) as other:
        with pytest.raises(RuntimeError, match="n rows"):
            other.add_hamming_self(idx, 0, 1, 0)
    with lib.Components(n) as cc:
        for row0, nrows, radius in ((-1, 1, 0), (0, n + 1, 0), (n, 1, 0), (n + 1, 0, 0), (5, -1, 0), (0, 1, -1)):
            with pytest.raises(RuntimeError):
                cc.add_hamming_self(idx, row0, nrows, radius)
        cc.add_hamming_self(idx, n, 0, 0)                      # an empty window at the end is fine
        assert cc.labels()[1] == n
    with pytest.raises(ValueError):
        near_duplicate_groups_hamming(idx, 1, batch=0)


# ---- 6. end to end: near-duplicate groups into the grouped search
def test_groups_collapse_in_the_grouped_search(lib):
    from isehr_amd.dedup import near_duplicate_groups
    n, d, nq, k = 300, 64, 20, 10
    X, rng = _float_rows_with_copies(61, n, d)
    Q = lt.dense_queries(rng, nq, d)
    S = lt.int_scores(X, X)
    tau = int(np.diag(S).min())
    i, j = np.nonzero(np.triu(S >= tau, 1))
    want_labels, want_groups = components_truth(n, i, j)
    assert want_groups <= n - 30
    with lib.Gallery.from_host(X, norm_mode=lib.NORM_NONE) as g:
        labels, G = near_duplicate_groups(g, tau)
        assert np.array_equal(labels, want_labels) and G == want_groups
        g.set_groups(labels)
        assert g.group_count() == G
        idx, sc, _, lab = g.search_grouped(Q, k, return_labels=True)
        for ids, scores in (gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)):
            wi, ws, wl = gt.grouped_truth(ids, scores, want_labels, k)
            assert np.array_equal(idx, wi) and np.array_equal(sc.view(np.uint32), ws.view(np.uint32)) and np.array_equal(lab, wl)
        for q in range(nq):                                    # no group twice in an answer
            assert len(set(lab[q].tolist())) == k


# ---- 7. Python plumbing
def test_any_integer_arrays(lib):
    n = 400
    rng = np.random.default_rng(71)
    i, j = rng.integers(0, n, 900), rng.integers(0, n, 900)
    want = components_truth(n, i, j)
    wide = np.stack([i, j, i], axis=1)                         # columns of a row-major matrix: strided
    forms = [(i.astype(np.int64), j.astype(np.int64)), (i.astype(np.int32), j.astype(np.int32)), (i.astype(np.uint16), j.astype(np.uint64)),
             (wide[:, 0], wide[:, 1]), (np.repeat(i, 2)[::2], np.repeat(j, 2).astype(np.int32)[::2]), (i.tolist(), j.tolist())]
    with lib.Components(n) as cc:
        for a, b in forms:
            cc.reset()
            cc.add_pairs(a, b)
            labels, groups = cc.labels()
            assert np.array_equal(labels, want[0]) and groups == want[1]
        with pytest.raises(ValueError):
            cc.add_pairs(i, j[:-1])
        with pytest.raises(ValueError):
            cc.add_pairs(i.astype(np.float32), j)
    ci, cj = csr_pairs(0, [0, 2, 2, 3], [1, 2, 3])
    with lib.Components(5) as cc:
        cc.add_csr(0, np.array([0, 2, 2, 3], dtype=np.int32), [1, 2, 3])
        assert np.array_equal(cc.labels()[0], components_truth(5, ci, cj)[0]) and cc.labels()[1] == 2
