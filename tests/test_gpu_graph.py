"""GPU: the graph index (mi_graph_search*, mi_graph_build, GraphIndex, matching_HNSW_hip) against the truth of
tests/_graph_truth.py, bit for bit: ids, float64 values and the number of rows evaluated.  The truth takes its values from
mi_refine (cross-checked against mi_knn_dense64_search_l2), so exact ties are part of what is tested."""
import os

import numpy as np
import pytest

import _graph_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _gallery(lib, rows, l2, off=0):
    if l2:
        return lib.Gallery.l2_from_host(rows, row_offset=off)
    return lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE, row_offset=off)


def _check_search(lib, g, q, table, entries, k, ef, l2):
    """Host search of `q` on a graph made of (table, entries) == the truth; -> (ids, values64, visited)."""
    want_ids, want_val, want_vis = T.search_truth(T.value_matrix(g, q, l2), table, entries, k, ef, l2, g.row_offset)
    with lib.GraphIndex.from_neighbors(g, table, entries) as gi:
        assert (gi.n, gi.R, gi.n_entry) == (g.n, table.shape[1], len(entries))
        ids, val64, secs, vis = gi.search(q, k, ef=ef, return_visited=True, return_values64=True)
        _, val32, _ = gi.search(q, k, ef=ef)
    assert secs > 0
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(val64, want_val)                # (no NaN in these inputs; padding is +-inf on both sides)
    assert np.array_equal(vis, want_vis)
    assert np.array_equal(val32, want_val.astype(np.float32))
    return ids, val64, vis


@pytest.mark.parametrize("case", T.sweep_cases(), ids=lambda c: "n%d-d%d-R%d-ef%d-%s-q%d-e%d-%s-off%d" % (
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], "l2" if c[7] else "ip", c[8]))
def test_search_equals_the_truth(lib, case):
    n, d, R, ef, kmode, nq, ne, l2, off = case
    rows, q, table, entries = T.case_inputs(case)
    g = _gallery(lib, rows, l2, off)
    try:
        _check_search(lib, g, q, table, entries, T.k_of(ef, kmode), ef, l2)
    finally:
        g.close()


@pytest.mark.parametrize("l2", [True, False])
def test_ties_are_broken_by_id(lib, l2):
    """40 distinct rows stored 8 times each; a query equal to a stored row (distance 0.0 exactly, eight times over) and ef below
    the size of a tie class."""
    rng = np.random.default_rng(7)
    base = rng.standard_normal((40, 24)).astype(np.float32)
    rows = np.tile(base, (8, 1))                         # row i == row i + 40 == ...
    q = np.concatenate([base[[3, 17]], rng.standard_normal((3, 24)).astype(np.float32)])
    table = T.random_table(rng, 320, 16)
    entries = np.array([5, 100, 319], np.int32)
    g = _gallery(lib, rows, l2)
    try:
        for ef, k in [(5, 5), (7, 3), (64, 64)]:
            ids, val, _ = _check_search(lib, g, q, table, entries, k, ef, l2)
        vals = T.value_matrix(g, q, l2)
        best = np.sort(vals if l2 else -vals, axis=1)
        assert (best[:, :8] == best[:, :1]).all()            # every query's best value comes eight times over
        if l2:
            assert (vals[0, 3::40] == 0.0).all()
    finally:
        g.close()


def test_ring_with_ef_n_is_the_exact_search(lib):
    rng = np.random.default_rng(11)
    n, d, k = 700, 33, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((6, d)).astype(np.float32)
    i = np.arange(n)
    ring = np.stack([(i - 1) % n, (i + 1) % n], axis=1).astype(np.int32)
    g = _gallery(lib, rows, True, off=50)
    try:
        want_ids, _, want_d64, _, _ = g.search_l2(q, k)
        with lib.GraphIndex.from_neighbors(g, ring, [123]) as gi:
            ids, val64, _, vis = gi.search(q, k, ef=n, return_visited=True, return_values64=True)
        assert np.array_equal(ids, want_ids) and np.array_equal(val64, want_d64)
        assert (vis == n).all()
        # two disjoint rings, entries in the first only: its rows and nothing else, padding beyond its size
        half = 300
        a, b = np.arange(half), np.arange(half, n)
        two = np.empty((n, 2), np.int32)
        two[a] = np.stack([(a - 1) % half, (a + 1) % half], axis=1)
        two[b] = np.stack([half + (b - half - 1) % (n - half), half + (b - half + 1) % (n - half)], axis=1)
        ids, val64, vis = _check_search(lib, g, q, two, np.array([7, 250], np.int32), 400, 400, True)
        assert ((ids[:, :half] >= 50) & (ids[:, :half] < 50 + half)).all()
        assert (ids[:, half:] == -1).all() and np.isinf(val64[:, half:]).all() and (vis == half).all()
    finally:
        g.close()


def test_malformed_table_terminates(lib):
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((500, 8)).astype(np.float32)
    q = rng.standard_normal((4, 8)).astype(np.float32)
    table = np.zeros((500, 4), np.int32)                 # every row points to row 0, four times
    g = _gallery(lib, rows, True)
    try:
        _, _, vis = _check_search(lib, g, q, table, np.array([9, 400, 9], np.int32), 8, 64, True)
        assert (vis == 3).all()
    finally:
        g.close()


def _clustered(rng, n, d, centers=20, spread=0.05):
    c = rng.standard_normal((centers, d)).astype(np.float32)
    return (c[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d))).astype(np.float32)


def _build_cases():
    rng = np.random.default_rng(17)
    dup = rng.standard_normal((60, 12)).astype(np.float32)
    dup[10:25] = dup[10]                                 # 15 identical rows, more than R + 1 = 9
    return [("n2", rng.standard_normal((2, 5)).astype(np.float32), 4, 3, True),
            ("n=R", rng.standard_normal((8, 7)).astype(np.float32), 8, 64, True),
            ("n=R+1", rng.standard_normal((9, 7)).astype(np.float32), 8, 2, False),
            ("clustered", _clustered(rng, 600, 16), 16, 16, True),
            ("clustered-ip", _clustered(rng, 300, 9), 6, 5, False),
            ("identical", dup, 8, 4, True),
            ("R64", rng.standard_normal((200, 3)).astype(np.float32), 64, 1, True)]


@pytest.mark.parametrize("name,rows,R,ne,l2", _build_cases(), ids=[c[0] for c in _build_cases()])
def test_build_equals_the_truth(lib, name, rows, R, ne, l2):
    import torch
    g = _gallery(lib, rows, l2, off=1000)
    try:
        want_table, want_entries = T.build_truth(T.value_matrix(g, rows, l2), R, ne, l2)
        with lib.GraphIndex.build(g, R=R, n_entry=ne) as gi, lib.GraphIndex.build(g, R=R, n_entry=ne) as again:
            table, entries = gi.neighbors, gi.entries
            assert table.dtype == np.int32 and table.shape == (g.n, R) and entries.dtype == np.int32
            assert np.array_equal(table, want_table)
            assert np.array_equal(entries, want_entries)
            assert table.tobytes() == again.neighbors.tobytes() and entries.tobytes() == again.entries.tobytes()
            # the host path and search_device agree bit for bit, and both are the truth on the built table
            q = np.ascontiguousarray(rows[::max(1, len(rows) // 7)] + np.float32(0.01))
            k, ef = min(5, g.n), 9
            ids, val64, _, vis = gi.search(q, k, ef=ef, return_visited=True, return_values64=True)
            want = T.search_truth(T.value_matrix(g, q, l2), table, entries, k, ef, l2, g.row_offset)
            assert np.array_equal(ids, want[0]) and np.array_equal(val64, want[1]) and np.array_equal(vis, want[2])
            tq = torch.from_numpy(q).cuda()
            didx = torch.full((len(q), k), -7, dtype=torch.int64, device="cuda")
            dv32 = torch.zeros((len(q), k), dtype=torch.float32, device="cuda")
            dv64 = torch.zeros((len(q), k), dtype=torch.float64, device="cuda")
            dvis = torch.zeros(len(q), dtype=torch.int32, device="cuda")
            gi.search_device(tq.data_ptr(), len(q), k, didx.data_ptr(), ef=ef, val_ptr=dv32.data_ptr(), val64_ptr=dv64.data_ptr(),
                             visited_ptr=dvis.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(didx.cpu().numpy(), ids) and dv64.cpu().numpy().tobytes() == val64.tobytes()
            assert np.array_equal(dv32.cpu().numpy(), val64.astype(np.float32)) and np.array_equal(dvis.cpu().numpy(), vis)
    finally:
        g.close()


def test_a_changed_gallery_makes_the_graph_stale(lib):
    rng = np.random.default_rng(19)
    rows = rng.standard_normal((64, 6)).astype(np.float32)
    q = rows[:2].copy()
    for change in ("remove", "append"):
        g = lib.Gallery.l2_from_host(rows, capacity=80)
        try:
            with lib.GraphIndex.build(g, R=4, n_entry=2) as gi:
                gi.search(q, 2)
                if change == "remove":
                    g.remove(np.array([5, 6]))
                else:
                    g.append(rows[:3])
                out = np.full((2, 2), -7, np.int64)
                rc = lib.load().mi_graph_search(gi._h, q.ctypes.data, 2, lib.MI_F32, 6, 1, 2, 8, out.ctypes.data, None, None, None,
                                                None)
                assert rc == lib.MI_ERR_INVALID and b"graph" in lib.load().mi_last_error()
                assert (out == -7).all()
                with pytest.raises(RuntimeError):
                    gi.search(q, 2)
        finally:
            g.close()


def test_matching_hnsw_hip(lib, tmp_path, monkeypatch):
    from isehr_amd import nnsearch
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(23)
    train = _clustered(rng, 2000, 32, centers=40, spread=0.2)
    test = train[rng.integers(0, 2000, 20)] + np.float32(0.01) * rng.standard_normal((20, 32)).astype(np.float32)
    K, m = 10, 16
    idx, per_query = nnsearch.matching_HNSW_hip(K, train, test, "demo/set", m=m, ifgenerate=True)
    assert idx.shape == (20, K) and idx.dtype == np.int64 and per_query > 0
    assert ((idx >= 0) & (idx < 2000)).all() and all(len(set(r)) == K for r in idx.tolist())
    path = os.path.join("outputs", "demo_set", "mi355_graph_R%d.npz" % (2 * m))
    assert os.path.exists(path) and not [f for f in os.listdir(os.path.dirname(path)) if ".tmp." in f]
    # persistence round trip: the loaded graph answers as the built one did
    again, _ = nnsearch.matching_HNSW_hip(K, train, test, "demo/set", m=m, ifgenerate=False)
    assert np.array_equal(idx, again)
    with pytest.raises(FileNotFoundError):
        nnsearch.matching_HNSW_hip(K, train, test, "demo/other", m=m, ifgenerate=False)
    # every returned id's distance is what the L2 gallery reports for it, ascending; some query's first hit is its exact nearest row
    g = lib.Gallery.l2_from_host(train)
    try:
        exact_ids, _, exact_d64, _, _ = g.search_l2(test, K)
        _, _, d64, _ = g.refine(test, idx, K)
        with np.load(path) as z:
            with lib.GraphIndex.from_neighbors(g, z["neighbors"], z["entries"]) as gi:
                ids, val64, _ = gi.search(test, K, ef=K, return_values64=True)
        assert np.array_equal(ids, idx) and np.array_equal(val64, d64)
        assert (np.diff(val64, axis=1) >= 0).all()
        assert (idx[:, 0] == exact_ids[:, 0]).any()
    finally:
        g.close()
    # the tail-filling rule on a disconnected table: rows 0 .. 3 are a component of their own, every entry lies in it
    small = train[:50]
    table = np.full((50, 2 * m), -1, np.int32)
    table[:4, 0] = [1, 2, 3, 0]
    os.makedirs(os.path.join("outputs", "tiny"), exist_ok=True)
    np.savez(os.path.join("outputs", "tiny", "mi355_graph_R%d.npz" % (2 * m)), neighbors=table, entries=np.array([0, 2], np.int32))
    idx, _ = nnsearch.matching_HNSW_hip(8, small, small[10:12], "tiny", m=m, ifgenerate=False)
    assert sorted(idx[0, :4].tolist()) == [0, 1, 2, 3] and idx[:, 4:].tolist() == [[4, 5, 6, 7]] * 2


@pytest.mark.parametrize("l2", [True, False])
def test_a_full_candidate_list_overflows_exactly(lib, l2):
    """ef = 2048 on 3000 well-connected rows: W fills up (eight places per thread in the merge) and pushes rows out."""
    rng = np.random.default_rng(29)
    rows = rng.standard_normal((3000, 5)).astype(np.float32)
    q = rng.standard_normal((2, 5)).astype(np.float32)
    g = _gallery(lib, rows, l2, off=77)
    try:
        _, _, vis = _check_search(lib, g, q, T.random_table(rng, 3000, 32), np.array([0, 1500, 2999], np.int32), 2048, 2048, l2)
        assert (vis > 2048).all()
    finally:
        g.close()
