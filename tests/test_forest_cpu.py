"""CPU: the random-projection forest (mi_forest*) is declared, exported and bound, answers bad arguments before
touching a device -- through the loaded library, through ForestIndex and through matching_ANNOY_hip --, and its truth
(tests/_forest_truth.py) does what the contract says on trees written out by hand here.
The library's checks that need the gallery's n or d (`2^L`, `candidates per query`, `leaf values`, `finite`) cannot answer through
a handle that is never read; they are asserted on a real gallery in tests/test_gpu_forest.py and, on this side, through the
Python surface, which applies the same rules before the library is called."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _forest_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mi_forest_build": 5, "mi_forest_create": 8, "mi_forest_info": 6, "mi_forest_get_splits": 4, "mi_forest_get_leaves": 4,
       "mi_forest_get_dirs": 2, "mi_forest_destroy": 1, "mi_forest_candidates": 8, "mi_forest_candidates_device": 5,
       "mi_forest_search": 11, "mi_forest_search_device": 8}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


class _NoDevice:
    """Stands where a Gallery would: any use of its handle fails the test."""
    n, d, row_offset, device = 10, 4, 0, 0

    @property
    def _h(self):
        raise AssertionError("the handle was used")

    _lock = _h


def test_symbols_are_declared_exported_and_bound(built_lib):
    lib, _lib = built_lib
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    for name, nargs in NEW.items():
        assert "int %s(" % name in hdr, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for meth in ("build", "from_trees", "search", "search_device", "candidates", "splits", "leaves", "dirs", "close", "__enter__",
                 "__exit__"):
        assert hasattr(_lib.ForestIndex, meth), meth
    p = inspect.signature(_lib.ForestIndex.build).parameters
    assert list(p) == ["gallery", "n_trees", "depth", "seed", "dirs"]
    assert p["n_trees"].default == 100 and p["depth"].default is None and p["seed"].default == 5 and p["dirs"].default is None
    assert list(inspect.signature(_lib.ForestIndex.from_trees).parameters) == ["gallery", "dirs", "splits", "leaves"]
    from isehr_amd import build
    for src in ("api_forest.hip", "forest_project.hip", "forest_build.hip", "forest_search.hip"):
        assert src in build.SOURCES
        assert os.path.exists(os.path.join(build.CSRC, src))


def test_matcher_is_registered_with_the_reference_signature():
    from isehr_amd import nnsearch
    assert nnsearch.MATCHING_METHODS["ANNOY"] is nnsearch.matching_ANNOY_hip
    p = inspect.signature(nnsearch.matching_ANNOY_hip).parameters
    assert list(p) == ["K", "embedded_features_train", "embedded_features_test", "metric", "dataset", "n_trees", "ifgenerate"]
    assert p["metric"].default == "euclidean" and p["dataset"].default is None and p["n_trees"].default == 100
    assert p["ifgenerate"].default is True
    assert "not the reference's" in nnsearch.matching_ANNOY_hip.__doc__


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    idx = np.zeros(16, np.int64)
    dirs = np.zeros((2, 4), np.float64)
    spl = np.zeros((2, 1), np.float64)
    lvs = np.zeros((2, 10), np.int32)
    out = C.c_void_p()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def dev(f=fake, qp=P(q), nq=2, k=4, op=P(idx)):
        return lib.mi_forest_search_device(f, qp, nq, k, op, None, None, None)

    def host(f=fake, qp=P(q), nq=2, dtype=0, k=4, op=P(idx)):
        return lib.mi_forest_search(f, qp, nq, dtype, 4, 1, k, op, None, None, None)

    for call in (dev, host):
        for kwargs, word in [(dict(f=None), b"null handle"), (dict(k=0), b"k must"), (dict(k=8193), b"k must"), (dict(nq=-1), b"nq"),
                             (dict(qp=None), b"queries"), (dict(op=None), b"out_idx")]:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
        assert call(nq=0, qp=None, op=None) == 0                  # nq == 0: MI_OK, nothing read, nothing written
    assert host(dtype=9) == _lib.MI_ERR_INVALID and b"dtype" in lib.mi_last_error()

    def cdev(f=fake, qp=P(q), nq=2, op=P(idx)):
        return lib.mi_forest_candidates_device(f, qp, nq, op, None)

    def chost(f=fake, qp=P(q), nq=2, dtype=0, op=P(idx)):
        return lib.mi_forest_candidates(f, qp, nq, dtype, 4, 1, op, None)

    for call in (cdev, chost):
        for kwargs, word in [(dict(f=None), b"null handle"), (dict(nq=-1), b"nq"), (dict(qp=None), b"queries"), (dict(op=None), b"out_cand")]:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
        assert call(nq=0, qp=None, op=None) == 0
    assert chost(dtype=9) == _lib.MI_ERR_INVALID and b"dtype" in lib.mi_last_error()
    assert (idx == 0).all()

    def build(g=fake, dp=P(dirs), T=2, L=1, o=C.byref(out)):
        return lib.mi_forest_build(g, dp, T, L, o)

    def create(g=fake, dp=P(dirs), T=2, L=1, sp=P(spl), lp=P(lvs), space=0, o=C.byref(out)):
        return lib.mi_forest_create(g, dp, T, L, sp, lp, space, o)

    common = [(dict(g=None), b"null handle"), (dict(dp=None), b"dirs"), (dict(o=None), b"out"), (dict(T=0), b"T must"),
              (dict(T=257), b"T must"), (dict(L=0), b"L must"), (dict(L=25), b"L must")]
    for call, cases in [(build, common), (create, common + [(dict(sp=None), b"splits"), (dict(lp=None), b"leaves"),
                                                            (dict(space=7), b"memspace")])]:
        for kwargs, word in cases:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
    assert out.value is None
    assert lib.mi_forest_info(None, None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_forest_get_splits(None, 0, 0, None) == _lib.MI_ERR_INVALID
    assert lib.mi_forest_get_leaves(None, 0, 0, None) == _lib.MI_ERR_INVALID
    assert lib.mi_forest_get_dirs(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_forest_destroy(None) == 0


def test_python_surface_raises_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd import nnsearch
    g = _NoDevice()                                           # n = 10, d = 4
    for kwargs, word in [(dict(n_trees=0), "T must"), (dict(n_trees=257), "T must"), (dict(n_trees=2, depth=0), "L must"),
                         (dict(n_trees=2, depth=25), "L must"), (dict(n_trees=2, depth=4), "2\\^L"),
                         (dict(n_trees=2, depth=1, dirs=np.zeros((3, 4))), "dirs"),
                         (dict(n_trees=2, depth=1, dirs=np.full((2, 4), np.inf)), "finite")]:
        with pytest.raises(ValueError, match=word):
            _lib.ForestIndex.build(g, **kwargs)
    big = _NoDevice()
    big.n = 100000
    with pytest.raises(ValueError, match="candidates per query"):
        _lib.ForestIndex.build(big, n_trees=100, depth=3)
    dirs, spl, lvs = np.zeros((2, 4)), np.zeros((2, 1)), np.zeros((2, 10), np.int64)
    bad = lvs.copy()
    bad[1, 3] = 10
    nan_dirs = dirs.copy()
    nan_dirs[0, 0] = np.nan
    for d_, s_, l_, word in [(dirs, spl, bad, "leaf values"), (dirs, spl, lvs - 1, "leaf values"), (dirs, spl, lvs[:, :9], "leaves of shape"),
                             (dirs, spl, lvs.astype(np.float32), "integer"), (dirs, np.zeros((2, 2)), lvs, "splits"),
                             (dirs, np.zeros((3, 1)), lvs, "splits"), (dirs, np.zeros((2, 15)), lvs, "2\\^L"),
                             (dirs[:1], spl, lvs, "dirs"), (nan_dirs, spl, lvs, "finite")]:
        with pytest.raises(ValueError, match=word):
            _lib.ForestIndex.from_trees(g, d_, s_, l_)
    # the depth ForestIndex.build picks
    assert _lib._forest_shape(None, 600, 100) == (4, 38)
    assert _lib._forest_shape(None, 2, 1) == (1, 1)
    assert _lib._forest_shape(None, 64, 1) == (1, 32) and _lib._forest_shape(None, 129, 3) == (2, 33)
    assert _lib._forest_shape(None, 10 ** 6, 100) == (14, 62) and _lib._forest_shape(None, 10 ** 6, 256) == (15, 31)
    assert _lib._forest_shape(3800, 600, 100) == (4, 38)
    for args, word in [((None, 1, 1), "no depth"), ((None, 65 * 2 ** 24, 1), "no depth"), ((None, 100, 0), "T must"),
                       ((None, 100, 257), "T must"), ((3801, 600, 100), "k = 3801")]:
        with pytest.raises(ValueError, match=word):
            _lib._forest_shape(*args)
    assert _lib.forest_directions(7, 3, 2).shape == (6, 7) and _lib.forest_directions(7, 3, 2).dtype == np.float64
    assert np.array_equal(_lib.forest_directions(7, 3, 2, seed=9), np.random.default_rng(9).standard_normal((6, 7)))
    train, test = np.zeros((20, 4), np.float32), np.zeros((3, 4), np.float32)
    for args, kwargs in [((0, train, test), {}), ((21, train, test), {}), ((5, train, test[:, :3]), {}), ((5, train, test), dict(n_trees=0)),
                         ((5, train, test), dict(n_trees=257)), ((5, train.astype(int), test), {}), ((1, train[:1], test), {}),
                         ((5, train, test), dict(metric="manhattan")), ((1, train, test), dict(ifgenerate=False)),
                         ((5, train, test), dict(metric="angular"))]:      # (angular: zero rows cannot be normalised)
        with pytest.raises(ValueError):
            nnsearch.matching_ANNOY_hip(*args, **kwargs)


def test_truth_builds_five_rows_as_written_out():
    """n = 5, L = 2, one tree.  Level 0 on column 0 = [3, 1, 4, 1, 5]: order (1, id 1), (1, id 3), (3, id 0), (4, id 2), (5, id 4);
    mid = floor(5 / 2) = 2, split = 3; children [1, 3] and [0, 2, 4].  Level 1 on column 1 = [9, 2, 7, 1, 8]: node (1, 0) owns
    [0, 2): (1, id 3), (2, id 1), mid = floor(5 / 4) = 1, split = 2; node (1, 1) owns [2, 5): (7, id 2), (8, id 4), (9, id 0),
    mid = floor(15 / 4) = 3, split = 8.  Leaves: [0, 1) [1, 2) [2, 3) [3, 5)."""
    P = np.array([[3.0, 9.0], [1.0, 2.0], [4.0, 7.0], [1.0, 1.0], [5.0, 8.0]])
    splits, leaves = T.build_truth(P, 1, 2)
    assert splits.tolist() == [[3.0, 2.0, 8.0]] and leaves.tolist() == [[3, 1, 2, 4, 0]]
    assert leaves.dtype == np.int32 and splits.dtype == np.float64
    assert T.leaf_max(5, 2) == 2
    # queries: (0, 0) -> left, left: leaf [0, 1) = row 3; (3, 2): ON both splits -> right, then node (1, 1): 2 < 8 -> left: leaf
    # [2, 3) = row 2; (3, 8) -> right, right: leaf [3, 5) = rows 4, 0; (nan, nan) -> left, left; (0, 2) -> left, ON the split -> right
    Pq = np.array([[0.0, 0.0], [3.0, 2.0], [3.0, 8.0], [np.nan, np.nan], [0.0, 2.0], [-0.0, 100.0]])
    cand = T.candidates_truth(Pq, splits, leaves, 5, 1, 2, row_offset=100)
    assert cand.tolist() == [[103, -1], [102, -1], [104, 100], [103, -1], [101, -1], [101, -1]]


def test_truth_lets_the_id_decide_a_tie_that_straddles_the_middle():
    """Six rows with the projections [2, 1, 1, 1, 1, 0] and L = 1: order (0, id 5), (1, id 1), (1, id 2), (1, id 3), (1, id 4),
    (2, id 0); mid = 3: rows 5, 1, 2 go left, rows 3, 4, 0 right, the split is the tie value.  A query exactly on it goes right.
    -0.0 ties with +0.0 and the id decides there too."""
    P = np.array([[2.0], [1.0], [1.0], [1.0], [1.0], [0.0]])
    splits, leaves = T.build_truth(P, 1, 1)
    assert splits.tolist() == [[1.0]] and leaves.tolist() == [[5, 1, 2, 3, 4, 0]]
    cand = T.candidates_truth(np.array([[1.0], [np.nextafter(1.0, 0.0)]]), splits, leaves, 6, 1, 1)
    assert cand.tolist() == [[3, 4, 0], [5, 1, 2]]
    splits, leaves = T.build_truth(np.array([[0.0], [-0.0], [0.0], [-0.0]]), 1, 1)
    assert leaves.tolist() == [[0, 1, 2, 3]] and splits[0, 0] == 0.0
    # two trees read their own columns: tree 1 on column L + l
    P2 = np.array([[0.0, 3.0], [1.0, 2.0], [2.0, 1.0], [3.0, 0.0]])
    splits, leaves = T.build_truth(P2, 2, 1)
    assert leaves.tolist() == [[0, 1, 2, 3], [3, 2, 1, 0]] and splits.tolist() == [[2.0], [2.0]]
    cand = T.candidates_truth(np.array([[0.0, 0.0]]), splits, leaves, 4, 2, 1, row_offset=10)
    assert cand.tolist() == [[10, 11, 13, 12]]


def test_truth_projects_in_float64_without_negative_zero():
    rows = np.array([[0.0, 1.0], [1.5, -2.0]], np.float32)
    dirs = np.array([[-3.0, 0.0], [1.0, 1.0]])
    P = T.project(rows, dirs)
    assert P.dtype == np.float64 and P.tolist() == [[0.0, 1.0], [-4.5, -0.5]]
    assert not np.signbit(P[0, 0])
    assert T.projection_bound(rows, dirs).tolist() == [[0.0, 4 * 2.0 ** -53], [4 * 2.0 ** -53 * 4.5, 4 * 2.0 ** -53 * 3.5]]


def test_sweep_covers_every_axis():
    cases = T.sweep_cases()
    assert len(cases) == 24 and len(set(cases)) == 24
    for axis, want in enumerate([T.NS, T.LS, T.TS, T.DS, T.KMODES, T.NQS, T.GALLERIES, T.OFFSETS, T.QMODES]):
        assert {c[axis] for c in cases} == set(want), axis
    for n, L, t, d, kmode, nq, gal, off, qmode in cases:
        assert (1 << L) <= n and t * T.leaf_max(n, L) <= 8192
    assert any(nq > (64 << 20) // (t * L * 8 + t * T.leaf_max(n, L) * 16) for n, L, t, d, _, nq, _, _, _ in cases)
