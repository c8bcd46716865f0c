"""CPU: the graph index (mi_graph*) is declared, exported and bound, answers bad arguments before touching a
device -- through the loaded library, through GraphIndex and through matching_HNSW_hip --, and its truth (tests/_graph_truth.py)
does what the contract says on three hand-made graphs whose traversal is written out here."""
import ctypes as C
import os

import numpy as np
import pytest

import _graph_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_graph_create", "mi_graph_build", "mi_graph_info", "mi_graph_get_neighbors", "mi_graph_get_entries", "mi_graph_destroy",
       "mi_graph_search", "mi_graph_search_device"]


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
    for name in NEW:
        assert "int %s(" % name in hdr, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
    assert len(_lib.SIGNATURES["mi_graph_search"][1]) == 13
    assert len(_lib.SIGNATURES["mi_graph_search_device"][1]) == 10
    for meth in ("build", "from_neighbors", "search", "search_device", "neighbors", "entries", "close", "__enter__", "__exit__"):
        assert hasattr(_lib.GraphIndex, meth), meth
    import inspect
    p = inspect.signature(_lib.GraphIndex.build).parameters
    assert p["R"].default == 32 and p["n_entry"].default == 16
    p = inspect.signature(_lib.GraphIndex.search).parameters
    assert p["ef"].default is None and p["return_visited"].default is False
    from isehr_amd import build
    for src in ("api_graph.hip", "graph_search.hip", "graph_build.hip"):
        assert src in build.SOURCES


def test_matcher_is_registered_with_the_reference_signature():
    import inspect
    from isehr_amd import nnsearch
    assert nnsearch.MATCHING_METHODS["HNSW"] is nnsearch.matching_HNSW_hip
    p = inspect.signature(nnsearch.matching_HNSW_hip).parameters
    assert list(p) == ["K", "embedded_features_train", "embedded_features_test", "dataset", "m", "ef", "ifgenerate"]
    assert p["m"].default == 4 and p["ef"].default == 8 and p["ifgenerate"].default is True and p["dataset"].default is None
    assert "not the reference's" in nnsearch.matching_HNSW_hip.__doc__


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    idx = np.zeros(16, np.int64)
    tab = np.zeros((10, 4), np.int32)
    ent = np.zeros(2, np.int32)
    out = C.c_void_p()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def dev(g=fake, qp=P(q), nq=2, k=4, ef=8, op=P(idx)):
        return lib.mi_graph_search_device(g, qp, nq, k, ef, op, None, None, None, None)

    def host(g=fake, qp=P(q), nq=2, dtype=0, k=4, ef=8, op=P(idx)):
        return lib.mi_graph_search(g, qp, nq, dtype, 4, 1, k, ef, op, None, None, None, None)

    for call in (dev, host):
        for kwargs, word in [(dict(g=None), b"null handle"), (dict(ef=0), b"ef must"), (dict(ef=2049, k=1), b"ef must"),
                             (dict(k=0), b"k must"), (dict(k=9), b"k must"), (dict(nq=-1), b"nq"), (dict(qp=None), b"queries"),
                             (dict(op=None), b"out_idx")]:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
        assert call(nq=0, qp=None, op=None) == 0                  # nq == 0: MI_OK, nothing read, nothing written
    assert host(dtype=9) == _lib.MI_ERR_INVALID and b"dtype" in lib.mi_last_error()
    assert (idx == 0).all()

    def build(g=fake, R=4, ne=2, o=C.byref(out)):
        return lib.mi_graph_build(g, R, ne, o)

    for kwargs, word in [(dict(g=None), b"null handle"), (dict(o=None), b"out"), (dict(R=3), b"R must be even"), (dict(R=0), b"R must"),
                         (dict(R=66), b"R must"), (dict(ne=0), b"ne must"), (dict(ne=65), b"ne must")]:
        assert build(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())

    def create(g=fake, tp=P(tab), R=4, space=0, ep=P(ent), ne=2, o=C.byref(out)):
        return lib.mi_graph_create(g, tp, R, space, ep, ne, o)

    bad_ent = np.array([0, -1], np.int32)
    for kwargs, word in [(dict(g=None), b"null handle"), (dict(tp=None), b"neighbors"), (dict(ep=None), b"entries"),
                         (dict(o=None), b"out"), (dict(R=0), b"R must"), (dict(R=66), b"R must"), (dict(ne=0), b"ne must"),
                         (dict(ne=65), b"ne must"), (dict(space=7), b"memspace"), (dict(ep=P(bad_ent)), b"entry rows")]:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert out.value is None
    assert lib.mi_graph_info(None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_graph_get_entries(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_graph_get_neighbors(None, 0, 0, None) == _lib.MI_ERR_INVALID
    assert lib.mi_graph_destroy(None) == 0


def test_python_surface_raises_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd import nnsearch
    g = _NoDevice()
    for kwargs, word in [(dict(R=3), "even"), (dict(R=0), "R must"), (dict(R=66), "R must"), (dict(n_entry=0), "entry rows"),
                         (dict(n_entry=65), "entry rows")]:
        with pytest.raises(ValueError, match=word):
            _lib.GraphIndex.build(g, **kwargs)
    tab, ent = np.zeros((10, 4), np.int64), np.array([0, 9])
    bad = tab.copy()
    bad[3, 1] = -2
    for t, e, word in [(bad, ent, "table values"), (tab + 10, ent, "table values"), (tab, np.array([10]), "entry rows"),
                       (tab, np.array([-1]), "entry rows"), (tab[:9], ent, "table of shape"), (np.zeros((10, 65), int), ent, "table"),
                       (tab, np.zeros(65, int), "entries of shape"), (tab.astype(np.float32), ent, "integer")]:
        with pytest.raises(ValueError, match=word):
            _lib.GraphIndex.from_neighbors(g, t, e)
    for k, ef, word in [(9, 8, "k must"), (0, 8, "k must"), (1, 2049, "ef must"), (1, 0, "ef must")]:
        with pytest.raises(ValueError, match=word):
            _lib._graph_search_shape(k, ef)
    assert _lib._graph_search_shape(10, None) == (10, 64) and _lib._graph_search_shape(100, None) == (100, 100)
    train, test = np.zeros((20, 4), np.float32), np.zeros((3, 4), np.float32)
    for args, kwargs in [((0, train, test), {}), ((21, train, test), {}), ((5, train, test[:, :3]), {}), ((5, train, test), dict(m=0)),
                         ((5, train, test), dict(m=33)), ((5, train.astype(int), test), {}), ((5, train[:1], test), {}),
                         ((1, train, test), dict(ifgenerate=False))]:
        with pytest.raises(ValueError):
            nnsearch.matching_HNSW_hip(*args, **kwargs)


def test_truth_walks_a_path_as_written_out():
    """Rows on a line at 0 .. 5, path graph i -> i - 1, i + 1, query at 3.2, entry row 0, ef = 2.
    start W = [0]; expand 0 -> 1: W = [1, 0]; expand 1 -> 2: W = [2, 1]; expand 2 -> 3: W = [3, 2]; expand 3 -> 4: W = [3, 4];
    expand 4 -> 5 (distance 1.8^2, pushed out): W = [3, 4], all expanded.  Six rows evaluated."""
    pos = np.arange(6, dtype=np.float64)
    vals = ((pos - 3.2) ** 2)[None, :]
    table = np.array([[-1, 1], [0, 2], [1, 3], [2, 4], [3, 5], [4, -1]])
    ids, val, vis = T.search_truth(vals, table, [0], 2, 2, True)
    assert ids.tolist() == [[3, 4]] and vis.tolist() == [6]
    assert val[0].tolist() == [vals[0, 3], vals[0, 4]]
    # ef = 1 walks the same path and keeps one row; the same walk as an inner-product search on negated values
    ids, _, vis = T.search_truth(vals, table, [0], 1, 1, True)
    assert ids.tolist() == [[3]] and vis.tolist() == [5]           # 0, 1, 2, 3, 4: row 4 is evaluated and loses, 5 never is
    ids, val, vis = T.search_truth(-vals, table, [0], 2, 2, False, row_offset=100)
    assert ids.tolist() == [[103, 104]] and vis.tolist() == [6] and val[0, 0] == -vals[0, 3]


def test_truth_breaks_ties_by_id_and_never_expands_what_it_pushed_out():
    """Star: row 0 points to 1 .. 4, all four at distance 1.0, row 0 at 4.0; rows 1 .. 3 point to row 5 (distance 0.0), row 4
    to row 6.  At ef = 2 only rows 1 and 2 stay in W: 3 and 4 are pushed out, stay visited and are never expanded.
    start W = [0]; expand 0: W = [1, 2] (ties by id; 0, 3, 4 pushed out); expand 1 -> 5: W = [5, 1] (2 pushed out); expand 5 (-> 3: visited);
    1 is expanded: stop.  Six rows evaluated, row 6 (reachable only through 4) never."""
    vals = np.array([[4.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.5]])
    table = np.array([[1, 2, 3, 4], [5, -1, -1, -1], [5, 5, 2, -1], [5, -1, -1, -1], [6, -1, -1, -1], [3, -1, -1, -1],
                      [-1, -1, -1, -1]])
    ids, val, vis = T.search_truth(vals, table, [0], 2, 2, True)
    assert ids.tolist() == [[5, 1]] and val.tolist() == [[0.0, 1.0]] and vis.tolist() == [6]
    # with room for everything the walk reaches row 6 too and orders the tie class by id
    ids, _, vis = T.search_truth(vals, table, [0, 0, 0], 7, 7, True)
    assert ids.tolist() == [[5, 6, 1, 2, 3, 4, 0]] and vis.tolist() == [7]


def test_truth_pads_a_component_and_builds_a_table_as_written_out():
    """Two disjoint pairs, entries in the first only: the answer holds its two rows and padding."""
    vals = np.array([[3.0, 2.0, 1.0, 0.0]])
    table = np.array([[1], [0], [3], [2]])
    ids, val, vis = T.search_truth(vals, table, [1, 1], 4, 4, True)
    assert ids.tolist() == [[1, 0, -1, -1]] and val.tolist() == [[2.0, 3.0, np.inf, np.inf]] and vis.tolist() == [2]
    # build: four rows on a line at 0, 1, 3, 7 with R = 2 (h = 1).  F = [[1, 2], [0, 2], [1, 0], [2, 1]];
    # B(0) = [1], B(1) = [0, 2], B(2) = [3], B(3) = [];  N(0) = [1] + [] (1 present) + [2]; N(1) = [0] + [2]; N(2) = [1] + [3];
    # N(3) = [2] + [] + [1]
    pos = np.array([0.0, 1.0, 3.0, 7.0])
    V = (pos[:, None] - pos[None, :]) ** 2
    table, entries = T.build_truth(V, 2, 3, True)
    assert table.tolist() == [[1, 2], [0, 2], [1, 3], [2, 1]] and entries.tolist() == [0, 1, 2]
    # five identical rows and R = 2: row 4 is not among its own three nearest (ids 0, 1, 2), so the last is dropped
    table, entries = T.build_truth(np.zeros((5, 5)), 2, 64, True)
    assert table.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]] and entries.tolist() == [0, 1, 2, 3, 4]
    table, _ = T.build_truth(V[:2, :2], 2, 1, True)
    assert table.tolist() == [[1, -1], [0, -1]]


def test_sweep_covers_every_axis():
    cases = T.sweep_cases()
    assert len(cases) == 40
    for axis, want in enumerate([T.NS, T.DS, T.RS, T.EFS, T.KMODES, T.NQS, T.NES, [True, False], [0, 1000003]]):
        assert {c[axis] for c in cases} == set(want), axis
