"""GPU: the random-projection forest (mi_forest*, ForestIndex, matching_ANNOY_hip) against the truth of
tests/_forest_truth.py: the candidate slots as arrays, the answer bit for bit against Gallery.refine on those slots and against the
float64 truth of tests/_refine_truth.py, the build byte for byte where every sum is exact and within the contract's error bound
where it is not."""
import ctypes as C
import os

import numpy as np
import pytest

import _forest_truth as T
import _refine_truth as R
from _graph_truth import gallery_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _gallery(lib, rows, kind, off=0, capacity=0):
    if kind == "l2":
        return lib.Gallery.l2_from_host(rows, row_offset=off, capacity=capacity)
    return lib.Gallery.from_host(rows, norm_mode={"norm_l2": lib.NORM_L2, "ip": lib.NORM_NONE}[kind], row_offset=off)


def _check_search(lib, g, f, q, cand, k, l2):
    """f.search(q, k) == Gallery.refine on `cand` bit for bit, and == the float64 truth on the first queries."""
    ids, val64, secs = f.search(q, k, return_values64=True)
    _, val32, _ = f.search(q, k)
    assert ids.shape == (len(q), k) and ids.dtype == np.int64
    if len(q) == 0:
        return ids
    assert secs > 0
    want_ids, want32, want64, _ = g.refine(q, cand, k)
    assert np.array_equal(ids, want_ids)
    assert val64.tobytes() == want64.tobytes() and val32.tobytes() == want32.tobytes()
    m = min(len(q), 6)
    stored, q32 = gallery_rows(g), np.asarray(q, np.float32)
    t_ids, t_val = R.refine_truth(stored, q32[:m], cand[:m], k, l2, g.row_offset)
    assert np.array_equal(t_ids >= 0, ids[:m] >= 0)
    with np.errstate(invalid="ignore"):
        err = np.where(ids[:m] >= 0, np.abs(val64[:m] - t_val), 0.0)
    assert (err <= R.value_bound(stored, q32[:m], ids[:m], g.d, g.row_offset)).all()
    if R.min_gap_over_bound(stored, q32[:m], cand[:m], l2, g.row_offset) > 2:
        assert np.array_equal(ids[:m], t_ids)
    return ids


@pytest.mark.parametrize("case", T.sweep_cases(), ids=lambda c: "n%d-L%d-T%d-d%d-%s-q%d-%s-off%d-%s" % c)
def test_descent_and_answer_on_given_trees(lib, case):
    n, L, Tn, d, kmode, nq, kind, off, qmode = case
    rows, q, dirs = T.case_inputs(case)
    g = _gallery(lib, rows, kind, off)
    try:
        stored = gallery_rows(g)
        splits, leaves = T.build_truth(T.project(stored, dirs), Tn, L)
        lm = T.leaf_max(n, L)
        with lib.ForestIndex.from_trees(g, dirs, splits, leaves) as f:
            assert (f.n, f.d, f.n_trees, f.depth, f.leaf_max) == (n, d, Tn, L, lm)
            assert f.splits().tobytes() == splits.tobytes() and f.leaves().tobytes() == leaves.tobytes()
            assert f.dirs().tobytes() == np.ascontiguousarray(dirs).tobytes()
            cand = f.candidates(q)
            want = T.candidates_truth(T.project(np.asarray(q, np.float32), dirs), splits, leaves, n, Tn, L, off)
            assert cand.dtype == np.int64 and cand.shape == (nq, Tn * lm)
            assert np.array_equal(cand, want)
            _check_search(lib, g, f, q, cand, T.k_of(Tn, lm, kmode), kind == "l2")
    finally:
        g.close()


@pytest.mark.parametrize("kind", ["l2", "norm_l2"])
def test_hand_made_trees_with_repeated_leaf_values(lib, kind):
    import torch
    rng = np.random.default_rng(31)
    n, d, Tn, L, off = 300, 7, 5, 3, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((9, d)).astype(np.float32)
    dirs = rng.standard_normal((Tn * L, d))
    splits = rng.standard_normal((Tn, 7)) * 0.5
    leaves = rng.integers(0, 20, size=(Tn, n)).astype(np.int32)       # twenty distinct rows, over and over
    lm = T.leaf_max(n, L)
    g = _gallery(lib, rows, kind, off)
    try:
        with lib.ForestIndex.from_trees(g, dirs, splits, leaves) as f:
            cand = f.candidates(q)
            assert np.array_equal(cand, T.candidates_truth(T.project(q, dirs), splits, leaves, n, Tn, L, off))
            ids = _check_search(lib, g, f, q, cand, 25, kind == "l2")
            assert (ids[:, 20:] == -1).all() and all(len(set(r[r >= 0])) == (r >= 0).sum() for r in ids)
            # the device forms agree with the host forms bit for bit
            k = 25
            tq = torch.from_numpy(q).cuda()
            dcand = torch.full((len(q), Tn * lm), -7, dtype=torch.int64, device="cuda")
            didx = torch.full((len(q), k), -7, dtype=torch.int64, device="cuda")
            dv32 = torch.zeros((len(q), k), dtype=torch.float32, device="cuda")
            dv64 = torch.zeros((len(q), k), dtype=torch.float64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            lib.check(lib.load().mi_forest_candidates_device(f._h, tq.data_ptr(), len(q), dcand.data_ptr(), s))
            f.search_device(tq.data_ptr(), len(q), k, didx.data_ptr(), val_ptr=dv32.data_ptr(), val64_ptr=dv64.data_ptr(), stream=s)
            torch.cuda.synchronize()
            _, val64, _ = f.search(q, k, return_values64=True)
            assert np.array_equal(dcand.cpu().numpy(), cand) and np.array_equal(didx.cpu().numpy(), ids)
            assert dv64.cpu().numpy().tobytes() == val64.tobytes()
            assert dv32.cpu().numpy().tobytes() == val64.astype(np.float32).tobytes()
    finally:
        g.close()


EXACT = [(2, 1, 1, 1), (64, 6, 3, 3), (65, 6, 100, 5), (65, 1, 3, 130), (64, 3, 100, 64), (1000, 3, 3, 1), (1000, 6, 100, 5),
         (1000, 1, 1, 64), (4097, 1, 3, 3), (4097, 6, 100, 130), (4097, 3, 1, 5),
         (3000, 10, 2, 5)]           # (ten levels: the node of a row takes two digits of the sort)


@pytest.mark.parametrize("n,L,Tn,d", EXACT, ids=["n%d-L%d-T%d-d%d" % c for c in EXACT])
def test_exact_build(lib, n, L, Tn, d):
    """Rows are integers in [-8, 8] and directions integers in [-4, 4]: every sum is exact in any order, ties abound, and the
    trees are the truth's byte for byte.  n == 2^L: every leaf holds one row; n == 2^L + 1: one leaf holds two."""
    rng = np.random.default_rng(1000 * n + 10 * L + d)
    rows = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    dirs = rng.integers(-4, 5, size=(Tn * L, d)).astype(np.float64)
    g = _gallery(lib, rows, "l2" if d % 2 else "ip", off=7)
    try:
        splits, leaves = T.build_truth(T.project(rows, dirs), Tn, L)
        with lib.ForestIndex.build(g, n_trees=Tn, depth=L, dirs=dirs) as f:
            assert f.leaf_max == T.leaf_max(n, L)
            got_s, got_l = f.splits(), f.leaves()
            assert got_l.dtype == np.int32 and got_l.shape == (Tn, n) and got_s.shape == (Tn, (1 << L) - 1)
            assert got_l.tobytes() == leaves.tobytes()
            assert got_s.tobytes() == splits.tobytes()
    finally:
        g.close()


def _check_gaussian_build(P, E, splits, leaves, Tn, L):
    """Every node's halves lie on their sides of the split, which is the projection of the row at the node's middle.  P: numpy's
    float64 projections; E: the contract's bound per projection.  The device's sum and numpy's each lie within the bound of the
    exact sum, so two values the device ordered a <= b satisfy P[a] <= P[b] + 2 (E[a] + E[b]), and a value the device copied lies
    within 2 E of numpy's."""
    n = P.shape[0]
    for t in range(Tn):
        assert np.array_equal(np.sort(leaves[t]), np.arange(n))
        for l in range(L):
            c = t * L + l
            for j in range(1 << l):
                a, b, mid = (j * n) >> l, ((j + 1) * n) >> l, ((2 * j + 1) * n) >> (l + 1)
                # the children's slices hold the node's rows whatever the deeper levels did to their order; the split is the
                # device's own projection of a right row, copied, so it carries no error of its own
                left, right = leaves[t][a:mid], leaves[t][mid:b]
                s = splits[t, (1 << l) - 1 + j]
                assert (np.abs(s - P[right, c]) <= 2 * E[right, c]).any()            # the split is some right row's projection
                assert (s <= P[right, c] + 2 * E[right, c]).all()                    # ... the smallest of the right child
                assert (P[left, c] - 2 * E[left, c] <= s).all()                      # and no left row lies above it
    # the last level leaves its order in the tree: leaves[t][mid] of a last-level node is the row the split was read from
    for t in range(Tn):
        c = t * L + L - 1
        for j in range(1 << (L - 1)):
            mid = ((2 * j + 1) * n) >> L
            r = leaves[t][mid]
            assert abs(splits[t, (1 << (L - 1)) - 1 + j] - P[r, c]) <= 2 * E[r, c]


def test_build_on_gaussian_rows(lib):
    rng = np.random.default_rng(37)
    for n, d, Tn, L, kind in [(1000, 33, 5, 4, "l2"), (4097, 130, 3, 6, "norm_l2"), (65, 5, 100, 6, "l2")]:
        rows = rng.standard_normal((n, d)).astype(np.float32)
        g = _gallery(lib, rows, kind)
        try:
            with lib.ForestIndex.build(g, n_trees=Tn, depth=L, seed=11) as f, lib.ForestIndex.build(g, n_trees=Tn, depth=L, seed=11) as again:
                dirs, splits, leaves = f.dirs(), f.splits(), f.leaves()
                assert dirs.tobytes() == lib.forest_directions(d, Tn, L, seed=11).tobytes()
                assert splits.tobytes() == again.splits().tobytes() and leaves.tobytes() == again.leaves().tobytes()
                stored = gallery_rows(g)
                _check_gaussian_build(T.project(stored, dirs), T.projection_bound(stored, dirs), splits, leaves, Tn, L)
        finally:
            g.close()


def test_grouping_of_trees_does_not_show(lib):
    """T = 40 in one build == the same directions built in slices of 8 trees == a build whose scratch holds three trees at a time."""
    rng = np.random.default_rng(41)
    n, d, Tn, L = 1000, 16, 40, 3
    rows = rng.standard_normal((n, d)).astype(np.float32)
    dirs = lib.forest_directions(d, Tn, L, seed=3)
    g = _gallery(lib, rows, "l2")
    try:
        with lib.ForestIndex.build(g, n_trees=Tn, depth=L, dirs=dirs) as f:
            splits, leaves = f.splits(), f.leaves()
        for t0 in range(0, Tn, 8):
            with lib.ForestIndex.build(g, n_trees=8, depth=L, dirs=dirs[t0 * L:(t0 + 8) * L]) as part:
                assert part.splits().tobytes() == splits[t0:t0 + 8].tobytes()
                assert part.leaves().tobytes() == leaves[t0:t0 + 8].tobytes()
        per_tree = n * (8 * L + 12) + 1024                      # the header's figure at n <= 2048
        lib.set_global_option("forest_build_bytes", 3 * per_tree + 100)
        try:
            with lib.ForestIndex.build(g, n_trees=Tn, depth=L, dirs=dirs) as small:
                assert small.splits().tobytes() == splits.tobytes() and small.leaves().tobytes() == leaves.tobytes()
        finally:
            lib.set_global_option("forest_build_bytes", 0)
        assert lib.get_global_option("forest_build_bytes") == float(1 << 30)
    finally:
        g.close()


def test_a_stored_row_finds_itself_in_every_tree(lib):
    """One kernel projects rows and queries: a query equal to a stored row descends every tree into that row's own leaf."""
    rng = np.random.default_rng(43)
    n, d, Tn = 1000, 33, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    g = _gallery(lib, rows, "l2", off=500)
    try:
        with lib.ForestIndex.build(g, n_trees=Tn) as f:
            assert (f.depth, f.leaf_max) == (4, 63)
            ids, val64, _ = f.search(rows, 1, return_values64=True)
            assert np.array_equal(ids[:, 0], 500 + np.arange(n)) and (val64 == 0.0).all()
            cand = f.candidates(rows).reshape(n, Tn, f.leaf_max)
            assert ((cand == (500 + np.arange(n))[:, None, None]).sum(axis=2) == 1).all()
    finally:
        g.close()


def test_a_changed_gallery_makes_the_forest_stale(lib):
    rng = np.random.default_rng(47)
    rows = rng.standard_normal((64, 6)).astype(np.float32)
    q = rows[:2].copy()
    for change in ("remove", "append"):
        g = lib.Gallery.l2_from_host(rows, capacity=80)
        try:
            with lib.ForestIndex.build(g, n_trees=4, depth=3) as f:
                f.search(q, 2)
                if change == "remove":
                    g.remove(np.array([5, 6]))
                else:
                    g.append(rows[:3])
                out = np.full((2, 2), -7, np.int64)
                cand = np.full((2, 32), -7, np.int64)
                rc = lib.load().mi_forest_search(f._h, q.ctypes.data, 2, lib.MI_F32, 6, 1, 2, out.ctypes.data, None, None, None)
                assert rc == lib.MI_ERR_INVALID and b"forest" in lib.load().mi_last_error()
                rc = lib.load().mi_forest_candidates(f._h, q.ctypes.data, 2, lib.MI_F32, 6, 1, cand.ctypes.data, None)
                assert rc == lib.MI_ERR_INVALID and b"forest" in lib.load().mi_last_error()
                assert (out == -7).all() and (cand == -7).all()
                with pytest.raises(RuntimeError):
                    f.search(q, 2)
                with pytest.raises(RuntimeError):
                    f.candidates(q)
        finally:
            g.close()


def test_checks_that_need_the_gallery(lib):
    """`2^L`, `candidates per query`, `leaf values`, `finite` and the upper end of `k must` read n, d or the forest's shape: they
    answer on a real gallery, before anything is allocated."""
    rng = np.random.default_rng(53)
    n = 20000
    rows = rng.standard_normal((n, 4)).astype(np.float32)
    g = lib.Gallery.l2_from_host(rows)
    L_ = lib.load()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        out = C.c_void_p()
        dirs = np.ones((32, 4))
        for T_, L, word in [(1, 15, b"2^L"), (2, 1, b"candidates per query")]:
            assert L_.mi_forest_build(g._h, P(dirs), T_, L, C.byref(out)) == lib.MI_ERR_INVALID
            assert word in L_.mi_last_error()
        bad = dirs.copy()
        bad[1, 2] = np.inf
        assert L_.mi_forest_build(g._h, P(bad), 2, 12, C.byref(out)) == lib.MI_ERR_INVALID and b"finite" in L_.mi_last_error()
        splits, leaves = np.zeros((2, 4095)), np.zeros((2, n), np.int32)
        leaves[1, n - 1] = n
        assert L_.mi_forest_create(g._h, P(dirs), 2, 12, P(splits), P(leaves), lib.MI_HOST, C.byref(out)) == lib.MI_ERR_INVALID
        assert b"leaf values" in L_.mi_last_error() and out.value is None
        with lib.ForestIndex.build(g, n_trees=2, depth=12) as f:
            assert f.leaf_max == 5
            idx = np.full((1, 11), -7, np.int64)
            assert L_.mi_forest_search(f._h, P(rows), 1, lib.MI_F32, 4, 1, 11, P(idx), None, None, None) == lib.MI_ERR_INVALID
            assert b"k must" in L_.mi_last_error() and (idx == -7).all()
            with pytest.raises(ValueError, match="k must"):
                f.search(rows[:1], 11)
            assert f.search(rows[:1], 10)[0].shape == (1, 10)
    finally:
        g.close()


def test_matching_annoy_hip(lib, tmp_path, monkeypatch):
    from isehr_amd import nnsearch
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(59)
    train = rng.standard_normal((600, 32)).astype(np.float32)
    test = train[rng.integers(0, 600, 20)] + np.float32(0.05) * rng.standard_normal((20, 32)).astype(np.float32)
    K = 10
    assert nnsearch.MATCHING_METHODS["ANNOY"] is nnsearch.matching_ANNOY_hip
    idx, per_query = nnsearch.MATCHING_METHODS["ANNOY"](K, train, test)
    assert idx.shape == (20, K) and idx.dtype == np.int64 and per_query > 0
    assert ((idx >= 0) & (idx < 600)).all() and all(len(set(r)) == K for r in idx.tolist())
    g = lib.Gallery.l2_from_host(train)
    try:
        with lib.ForestIndex.build(g, n_trees=100, seed=5) as f:
            assert (f.depth, f.leaf_max) == (4, 38)
            ids, _, _ = f.search(test, K)
        assert np.array_equal(idx, ids)
    finally:
        g.close()
    # persistence round trip: the loaded forest answers as the built one did
    first, _ = nnsearch.matching_ANNOY_hip(K, train, test, "euclidean", "demo/set", n_trees=100, ifgenerate=True)
    path = os.path.join("outputs", "demo_set", "mi355_forest_T100_L4.npz")
    assert os.path.exists(path) and not [p for p in os.listdir(os.path.dirname(path)) if ".tmp." in p]
    again, _ = nnsearch.matching_ANNOY_hip(K, train, test, "euclidean", "demo/set", n_trees=100, ifgenerate=False)
    assert np.array_equal(first, idx) and np.array_equal(again, idx)
    with pytest.raises(FileNotFoundError):
        nnsearch.matching_ANNOY_hip(K, train, test, "euclidean", "demo/other", ifgenerate=False)
    # angular == euclidean on pre-normalised inputs.  Dividing a float32 unit row by its norm once more may move a last bit, so
    # the euclidean call gets exactly the float32 rows the angular call stores
    tn, qn = nnsearch._l2_rows_f32(train, "train"), nnsearch._l2_rows_f32(test, "test")
    a, _ = nnsearch.matching_ANNOY_hip(K, tn, qn, "angular", n_trees=20)
    e, _ = nnsearch.matching_ANNOY_hip(K, nnsearch._l2_rows_f32(tn, "train"), nnsearch._l2_rows_f32(qn, "test"), "euclidean", n_trees=20)
    assert np.array_equal(a, e)
    assert (np.abs(np.linalg.norm(tn.astype(np.float64), axis=1) - 1) < 1e-6).all()
