"""GPU: the graph index over PQ codes (mi_pq_graph_search*, mi_pq_graph_build, mi_pq_decode, PQGraphIndex, the PQ + HNSW matchers;
DESIGN.md 5.16b) against the truth of tests/_pq_graph_truth.py, bit for bit: ids, float32 distances and the number of rows
evaluated.  The truth's values are those of the PQ search (tests/_pq_truth.py), so exact ties and +inf are part of what is
tested."""
import os

import numpy as np
import pytest

import _graph_truth as G
import _pq_graph_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _device_search(gi, q, k, ef):
    """search_device on float32 queries -> (ids, dist, visited) as numpy."""
    import torch
    nq = len(q)
    tq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
    didx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    ddist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    dvis = torch.zeros(nq, dtype=torch.int32, device="cuda")
    gi.search_device(tq.data_ptr(), nq, k, didx.data_ptr(), ef=ef, dist_ptr=ddist.data_ptr(), visited_ptr=dvis.data_ptr(),
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return didx.cpu().numpy(), ddist.cpu().numpy(), dvis.cpu().numpy()


def _check_search(lib, pq, C, codes, q, table, entries, k, ef):
    """Host and device search of `q` on a graph made of (table, entries) == the truth; -> (ids, dist, visited)."""
    want_ids, want_dist, want_vis = T.search_truth(q, C, codes, table, entries, k, ef, pq.row_offset)
    with lib.PQGraphIndex.from_neighbors(pq, table, entries) as gi:
        assert (gi.n, gi.R, gi.n_entry) == (pq.n, table.shape[1], len(entries))
        ids, dist, secs, vis = gi.search(q, k, ef=ef, return_visited=True)
        dev = _device_search(gi, q, k, ef) if q.dtype == np.float32 else None
        assert gi.hbm_bytes >= table.size * 4 + len(entries) * 4
    assert secs > 0
    assert np.array_equal(ids, want_ids)
    assert _same_bits(dist, want_dist)
    assert np.array_equal(vis, want_vis)
    if dev is not None:
        assert np.array_equal(dev[0], ids) and _same_bits(dev[1], dist) and np.array_equal(dev[2], vis)
    return ids, dist, vis


@pytest.mark.parametrize("case", T.sweep_cases(), ids=T.case_id)
def test_search_equals_the_truth(lib, case):
    """The sweep, and with its last case (M = 64, Ks = 256, ef = 2048, n = 3000) the largest LDS carve the contract admits."""
    n, d, M, Ks, R, ef, kmode, nq, ne, off = case
    C, codes, q, table, entries = T.case_inputs(case)
    with lib.PQIndex.from_codes(C, codes, row_offset=off) as pq:
        _check_search(lib, pq, C, codes, q, table, entries, G.k_of(ef, kmode), ef)


def test_two_distance_classes(lib):
    """Ks = 2, M = 1: 300 rows at two distances, every answer decided by the id."""
    rng = np.random.default_rng(3)
    C = rng.standard_normal((1, 2, 6)).astype(np.float32)
    codes = rng.integers(0, 2, size=(300, 1)).astype(np.uint8)
    q = rng.standard_normal((4, 6)).astype(np.float32)
    with lib.PQIndex.from_codes(C, codes) as pq:
        for ef, k in [(5, 5), (64, 7), (300, 300)]:
            _, dist, _ = _check_search(lib, pq, C, codes, q, G.random_table(rng, 300, 8), np.array([0, 150, 299], np.int32), k, ef)
            assert all(len(set(r) - {np.inf}) <= 2 for r in dist.tolist())       # (+inf: padding where W ran short of k)


def test_repeated_codes_and_zero_distances(lib):
    """Every code three times over, queries equal to a reconstruction (distance 0.0 exactly, three times), float64 queries too."""
    rng = np.random.default_rng(5)
    C = rng.standard_normal((4, 16, 3)).astype(np.float32)
    base = rng.integers(0, 16, size=(100, 4)).astype(np.uint8)
    codes = np.tile(base, (3, 1))
    q = np.concatenate([T.decode(C, base[[3, 40]]), rng.standard_normal((3, 12)).astype(np.float32)])
    table = G.random_table(rng, 300, 16)
    entries = np.array([5, 100, 299], np.int32)
    with lib.PQIndex.from_codes(C, codes) as pq:
        for ef, k in [(2, 2), (7, 3), (300, 300)]:
            ids, dist, _ = _check_search(lib, pq, C, codes, q, table, entries, k, ef)
        assert (dist[:2, :3] == 0.0).all() and ids[0, :3].tolist() == [3, 103, 203] and ids[1, :3].tolist() == [40, 140, 240]
        _check_search(lib, pq, C, codes, q.astype(np.float64) * 1.0000001, table, entries, 5, 9)


def test_infinite_table_entries_are_ordinary_values(lib):
    """A codeword near 3e38 against an ordinary query: its table entry is beyond float32, every row that uses it is at +inf."""
    rng = np.random.default_rng(7)
    C = rng.standard_normal((3, 7, 5)).astype(np.float32)
    C[1, 2, 4] = np.float32(3e38)
    codes = rng.integers(0, 7, size=(300, 3)).astype(np.uint8)
    q = rng.standard_normal((5, 15)).astype(np.float32)
    assert np.isinf(T.values(q, C, codes)).any()
    with lib.PQIndex.from_codes(C, codes, row_offset=9) as pq:
        _, dist, _ = _check_search(lib, pq, C, codes, q, G.random_table(rng, 300, 32), np.array([1, 2, 3], np.int32), 300, 300)
        assert np.isinf(dist).any() and not np.isnan(dist).any()
        _check_search(lib, pq, C, codes, q, G.random_table(rng, 300, 4), np.array([0], np.int32), 4, 16)


def _build_codes(rng, n, distinct):
    base = rng.integers(0, 16, size=(distinct or n, 4)).astype(np.uint8)
    return base if not distinct else base[rng.integers(0, distinct, n)]


@pytest.mark.parametrize("n", [2, 3, 65, 300])
@pytest.mark.parametrize("R", [2, 4, 64])
@pytest.mark.parametrize("distinct", [0, 3], ids=["random", "three-codes"])
def test_build_equals_the_truth(lib, n, R, distinct):
    """distinct = 3: whole classes of identical codes, larger than R + 1 from n = 65 on -- the row absent from its own list."""
    rng = np.random.default_rng([n, R, distinct])
    C = rng.standard_normal((4, 16, 2)).astype(np.float32)
    codes = _build_codes(rng, n, distinct)
    want_table, want_entries = T.build_truth(C, codes, R, 5)
    with lib.PQIndex.from_codes(C, codes, row_offset=1000) as pq:
        with lib.PQGraphIndex.build(pq, R=R, n_entry=5) as gi, lib.PQGraphIndex.build(pq, R=R, n_entry=5) as again:
            table, entries = gi.neighbors, gi.entries
            assert table.dtype == np.int32 and table.shape == (n, R) and entries.dtype == np.int32
            assert np.array_equal(table, want_table)
            assert np.array_equal(entries, want_entries)
            assert table.tobytes() == again.neighbors.tobytes() and entries.tobytes() == again.entries.tobytes()
            q = rng.standard_normal((3, 8)).astype(np.float32)
            k, ef = min(5, n), 9
            got = gi.search(q, k, ef=ef, return_visited=True)
            # get_neighbors / get_entries round-trip through from_neighbors: the same graph, the same answer, the truth
            want = _check_search(lib, pq, C, codes, q, table, entries, k, ef)
            assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]) and np.array_equal(got[3], want[2])


def test_malformed_tables_terminate(lib):
    rng = np.random.default_rng(13)
    C = rng.standard_normal((2, 7, 4)).astype(np.float32)
    codes = rng.integers(0, 7, size=(500, 2)).astype(np.uint8)
    q = rng.standard_normal((4, 8)).astype(np.float32)
    with lib.PQIndex.from_codes(C, codes) as pq:
        zero = np.zeros((500, 4), np.int32)                  # every row points to row 0, four times
        _, _, vis = _check_search(lib, pq, C, codes, q, zero, np.array([9, 400, 9], np.int32), 8, 64)
        assert (vis == 3).all()
        i = np.arange(500)
        ring = np.stack([(i + 1) % 500, (i + 1) % 500, i], axis=1).astype(np.int32)
        _, _, vis = _check_search(lib, pq, C, codes, q, ring, np.array([123], np.int32), 8, 500)
        assert (vis == 500).all()
        _check_search(lib, pq, C, codes, q, ring, np.array([123], np.int32), 2, 2)


def test_a_changed_index_makes_the_graph_stale(lib):
    rng = np.random.default_rng(19)
    C = rng.standard_normal((2, 8, 3)).astype(np.float32)
    codes = rng.integers(0, 8, size=(64, 2)).astype(np.uint8)
    rows = T.decode(C, codes)
    q = np.ascontiguousarray(rows[:2])
    for change in ("add", "append_codes", "remove-then-add"):
        with lib.PQIndex.from_codes(C, codes, capacity=80) as pq:
            with lib.PQGraphIndex.build(pq, R=4, n_entry=2) as gi:
                gi.search(q, 2)
                if change == "add":
                    pq.add(rows[:3])
                elif change == "append_codes":
                    pq.append_codes(codes[:3])
                else:
                    pq.remove(np.array([5, 6]))
                    pq.add(rows[5:7])
                    assert pq.n == gi.n == 64
                out = np.full((2, 2), -7, np.int64)
                rc = lib.load().mi_pq_graph_search(gi._h, q.ctypes.data, 2, lib.MI_F32, 6, 1, 2, 8, out.ctypes.data, None, None, None)
                assert rc == lib.MI_ERR_INVALID and b"graph" in lib.load().mi_last_error(), change
                assert (out == -7).all()
                with pytest.raises(RuntimeError):
                    _device_search(gi, q, 2, 8)
                with pytest.raises(RuntimeError):
                    gi.search(q, 2)
            with lib.PQGraphIndex.build(pq, R=4, n_entry=2) as fresh:          # a new graph over the changed index answers
                fresh.search(q, 2)


def test_the_pq_index_is_left_as_it_was(lib):
    rng = np.random.default_rng(23)
    C = rng.standard_normal((4, 16, 4)).astype(np.float32)
    codes = rng.integers(0, 16, size=(300, 4)).astype(np.uint8)
    q = rng.standard_normal((9, 16)).astype(np.float32)
    with lib.PQIndex.from_codes(C, codes, row_offset=5) as pq:
        ids0, dist0, _ = pq.search(q, 20)
        with lib.PQGraphIndex.build(pq, R=8, n_entry=4) as gi:
            gi.search(q, 10, ef=40)
            ids1, dist1, _ = pq.search(q, 20)
        ids2, dist2, _ = pq.search(q, 20)
        assert np.array_equal(ids0, ids1) and _same_bits(dist0, dist1) and np.array_equal(ids0, ids2) and _same_bits(dist0, dist2)
        assert np.array_equal(pq.get_codes(), codes) and pq.n == 300


@pytest.mark.parametrize("n,M,Ks,L", [(1, 1, 2, 1), (65, 3, 7, 5), (300, 16, 256, 4), (130, 64, 256, 2)])
def test_decode_is_the_gather(lib, n, M, Ks, L):
    rng = np.random.default_rng([n, M, Ks, L])
    C = rng.standard_normal((M, Ks, L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M)).astype(np.uint8)
    with lib.PQIndex.from_codes(C, codes) as pq:
        assert _same_bits(pq.decode(), T.decode(C, codes))
        lo, cnt = n // 3, n - n // 2
        assert _same_bits(pq.decode(lo, cnt), T.decode(C, codes[lo:lo + cnt]))
        assert pq.decode(n, 0).shape == (0, M * L)
        with pytest.raises(RuntimeError):
            pq.decode(1, n)


def test_a_chain_with_ef_n_is_the_exhaustive_search(lib):
    rng = np.random.default_rng(29)
    n = 700
    C = rng.standard_normal((3, 7, 4)).astype(np.float32)
    codes = rng.integers(0, 7, size=(n, 3)).astype(np.uint8)          # 343 distinct codes at the most: ties throughout
    q = rng.standard_normal((6, 12)).astype(np.float32)
    chain = np.minimum(np.arange(n) + 1, n - 1).astype(np.int32)[:, None]
    with lib.PQIndex.from_codes(C, codes, row_offset=50) as pq:
        want_ids, want_dist, _ = pq.search(q, n)
        with lib.PQGraphIndex.from_neighbors(pq, chain, [0]) as gi:
            ids, dist, _, vis = gi.search(q, n, ef=n, return_visited=True)
        assert np.array_equal(ids, want_ids) and _same_bits(dist, want_dist) and (vis == n).all()


def _clustered(rng, n, d, centers=20, spread=0.2):
    c = rng.standard_normal((centers, d)).astype(np.float32)
    return (c[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d))).astype(np.float32)


def _tail_filled(idx, n):
    out = idx.copy()
    for r in range(len(out)):
        got = [i for i in out[r].tolist() if i >= 0]
        out[r] = (got + [i for i in range(n) if i not in got])[:out.shape[1]]
    return out


def test_matchers(lib, tmp_path, monkeypatch):
    from isehr_amd import nnsearch
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(31)
    n, d, K, m, M, Ks = 300, 64, 10, 4, 8, 16
    train = _clustered(rng, n, d)
    test = train[rng.integers(0, n, 12)] + np.float32(0.01) * rng.standard_normal((12, d)).astype(np.float32)
    # ---- PQ_HNSW: learned codebooks, persisted with table and entries
    match = nnsearch.MATCHING_METHODS["PQ_HNSW"]
    idx, per_query = match(K, train, test, "demo/set", N_books=M, N_words=Ks, m=m, ifgenerate=True)
    assert idx.shape == (12, K) and idx.dtype == np.int64 and per_query > 0
    assert ((idx >= 0) & (idx < n)).all() and all(len(set(r)) == K for r in idx.tolist())
    path = os.path.join("outputs", "demo_set", "mi355_pqgraph_M%d_Ks%d_R%d.npz" % (M, Ks, 2 * m))
    assert os.path.exists(path) and not [f for f in os.listdir(os.path.dirname(path)) if ".tmp." in f]
    again, _ = match(K, train, test, "demo/set", N_books=M, N_words=Ks, m=m, ifgenerate=False)
    assert np.array_equal(idx, again)
    with pytest.raises(FileNotFoundError):
        match(K, train, test, "demo/other", N_books=M, N_words=Ks, m=m, ifgenerate=False)
    nodataset, _ = match(K, train, test, None, N_books=M, N_words=Ks, m=m)
    assert np.array_equal(idx, nodataset)
    tr32, te32 = nnsearch._l2_rows_f32(train, "train"), nnsearch._l2_rows_f32(test, "test")
    with np.load(path) as z:
        books, table, entries = z["codebooks"], z["neighbors"], z["entries"]
    assert books.shape == (M, Ks, d // M) and table.shape == (n, 2 * m) and len(entries) == 16
    with lib.PQIndex.empty(books, n) as pq:
        pq.add(tr32)
        codes = pq.get_codes()
        with lib.PQGraphIndex.from_neighbors(pq, table, entries) as gi:
            ids, _, _ = gi.search(te32, K, ef=K)
        with lib.PQGraphIndex.build(pq, R=2 * m, n_entry=16) as built:
            assert np.array_equal(built.neighbors, table) and np.array_equal(built.entries, entries)
    assert np.array_equal(idx, _tail_filled(ids, n))
    # ---- matching_HNSW_PQ_hip on the same codes, Codewords in the reference's layout [Ks, dim]
    codewords = np.ascontiguousarray(books.transpose(1, 0, 2)).reshape(Ks, d)
    idx2, per_query = nnsearch.matching_HNSW_PQ_hip(K, codewords, test, codes, m=m)
    assert idx2.shape == (12, K) and idx2.dtype == np.int64 and per_query > 0
    assert ((idx2 >= 0) & (idx2 < n)).all() and all(len(set(r)) == K for r in idx2.tolist())
    qn = test / np.linalg.norm(test, axis=1)[:, None]
    with lib.PQIndex.from_codes(books, codes) as pq, lib.PQGraphIndex.build(pq, R=2 * m, n_entry=16) as gi:
        ids2, _, _ = gi.search(qn, K, ef=K)
    assert np.array_equal(idx2, _tail_filled(ids2, n))
    # ---- the tail fill where the graph reaches fewer than K rows: rows 0 .. 3 are a component of their own
    table = np.full((n, 2 * m), -1, np.int32)
    table[:4, 0] = [1, 2, 3, 0]
    os.makedirs(os.path.join("outputs", "tiny"), exist_ok=True)
    np.savez(os.path.join("outputs", "tiny", os.path.basename(path)), codebooks=books, neighbors=table, entries=np.array([0, 2], np.int32))
    idx3, _ = match(8, train, test[:2], "tiny", N_books=M, N_words=Ks, m=m, ifgenerate=False)
    assert sorted(idx3[0, :4].tolist()) == [0, 1, 2, 3] and idx3[:, 4:].tolist() == [[4, 5, 6, 7]] * 2


def test_refine_composes_on_the_device(lib):
    rng = np.random.default_rng(37)
    n, d, k, f, ef = 300, 64, 5, 6, 12
    rows = _clustered(rng, n, d)
    q = rows[rng.integers(0, n, 7)] + np.float32(0.05) * rng.standard_normal((7, d)).astype(np.float32)
    with lib.PQIndex.fit(rows, 8, 16, row_offset=40) as pq, lib.PQGraphIndex.build(pq, R=8, n_entry=4) as gi:
        g = lib.Gallery.l2_from_host(rows, row_offset=40)
        try:
            kc = k * f
            short, _, _ = gi.search(q, kc, ef=max(ef, kc))          # (trailing -1s, if any, are padding to Gallery.refine)
            want_ids, want_val, _, _ = g.refine(q, short, k)
            ids, val, secs = gi.search(q, k, ef=ef, refine=g, k_factor=f)
            assert np.array_equal(ids, want_ids) and _same_bits(val, want_val) and secs > 0
            # the shortlist is capped by n and by the 2048 places a graph search has
            short, _, _ = gi.search(q, n, ef=n)
            want_ids, want_val, _, _ = g.refine(q, short, k)
            ids, val, _ = gi.search(q, k, ef=ef, refine=g, k_factor=1000)
            assert np.array_equal(ids, want_ids) and _same_bits(val, want_val)
            with pytest.raises(ValueError):
                gi.search(q, k, refine=g, return_visited=True)
        finally:
            g.close()
