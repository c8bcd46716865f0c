"""CPU: the graph index over PQ codes (mi_pq_graph*, mi_pq_decode) is declared, exported and bound, answers bad
arguments before touching a device -- through the loaded library, through PQGraphIndex and through the two matchers --, and its
truth (tests/_pq_graph_truth.py) is the brute-force ADC top-K where the table is complete."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _pq_graph_truth as T
import _pq_truth as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mi_pq_graph_create": 7, "mi_pq_graph_build": 4, "mi_pq_graph_info": 5, "mi_pq_graph_get_neighbors": 4,
       "mi_pq_graph_get_entries": 2, "mi_pq_graph_destroy": 1, "mi_pq_graph_search": 12, "mi_pq_graph_search_device": 9,
       "mi_pq_decode": 4}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


class _NoDevice:
    """Stands where a PQIndex would: any use of its handle fails the test."""
    n, d, m, ks, row_offset, device = 10, 4, 2, 4, 0, 0

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
    for meth in ("build", "from_neighbors", "search", "search_device", "neighbors", "entries", "hbm_bytes", "close", "__enter__",
                 "__exit__"):
        assert hasattr(_lib.PQGraphIndex, meth), meth
    p = inspect.signature(_lib.PQGraphIndex.build).parameters
    assert p["R"].default == 32 and p["n_entry"].default == 16
    p = inspect.signature(_lib.PQGraphIndex.search).parameters
    assert p["ef"].default is None and p["return_visited"].default is False and p["refine"].default is None
    assert p["k_factor"].default == 1
    p = inspect.signature(_lib.PQIndex.decode).parameters
    assert p["row0"].default == 0 and p["nrows"].default is None
    from isehr_amd import build
    for src in ("api_pq_graph.hip", "pq_graph_search.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))


def test_matchers_are_registered_with_the_reference_signatures():
    from isehr_amd import nnsearch
    assert nnsearch.MATCHING_METHODS["PQ_HNSW"] is nnsearch.matching_HNSW_NanoPQ_hip
    assert nnsearch.matching_HNSW_PQ_hip not in nnsearch.MATCHING_METHODS.values()
    p = inspect.signature(nnsearch.matching_HNSW_NanoPQ_hip).parameters
    assert list(p) == ["K", "embedded_features", "embedded_features_test", "dataset", "N_books", "N_words", "m", "ef", "ifgenerate"]
    assert (p["N_books"].default, p["N_words"].default, p["m"].default, p["ef"].default) == (16, 256, 4, 8)
    assert p["ifgenerate"].default is True and p["dataset"].default is None
    p = inspect.signature(nnsearch.matching_HNSW_PQ_hip).parameters
    assert list(p) == ["K", "Codewords", "embedded_features_test", "CW_idx", "m"] and p["m"].default == 4
    for f in (nnsearch.matching_HNSW_NanoPQ_hip, nnsearch.matching_HNSW_PQ_hip):
        assert "not the reference's" in f.__doc__ and "NOT de-duplicated" in f.__doc__


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    idx = np.zeros(16, np.int64)
    tab = np.zeros((10, 4), np.int32)
    ent = np.zeros(2, np.int32)
    out = C.c_void_p()
    P_ = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                          # non-null, never dereferenced: these checks answer before the handle is read

    def dev(g=fake, qp=P_(q), nq=2, k=4, ef=8, op=P_(idx)):
        return lib.mi_pq_graph_search_device(g, qp, nq, k, ef, op, None, None, None)

    def host(g=fake, qp=P_(q), nq=2, dtype=0, k=4, ef=8, op=P_(idx)):
        return lib.mi_pq_graph_search(g, qp, nq, dtype, 4, 1, k, ef, op, None, None, None)

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
        return lib.mi_pq_graph_build(g, R, ne, o)

    for kwargs, word in [(dict(g=None), b"null handle"), (dict(o=None), b"out"), (dict(R=3), b"R must be even"), (dict(R=0), b"R must"),
                         (dict(R=66), b"R must"), (dict(ne=0), b"ne must"), (dict(ne=65), b"ne must")]:
        assert build(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())

    def create(g=fake, tp=P_(tab), R=4, space=0, ep=P_(ent), ne=2, o=C.byref(out)):
        return lib.mi_pq_graph_create(g, tp, R, space, ep, ne, o)

    bad_ent = np.array([0, -1], np.int32)
    for kwargs, word in [(dict(g=None), b"null handle"), (dict(tp=None), b"neighbors"), (dict(ep=None), b"entries"),
                         (dict(o=None), b"out"), (dict(R=0), b"R must"), (dict(R=65), b"R must"), (dict(ne=0), b"ne must"),
                         (dict(ne=65), b"ne must"), (dict(space=7), b"memspace"), (dict(ep=P_(bad_ent)), b"entry rows")]:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert out.value is None
    assert lib.mi_pq_graph_info(None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_graph_get_entries(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_graph_get_neighbors(None, 0, 0, None) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_decode(None, 0, 0, None) == _lib.MI_ERR_INVALID and b"null handle" in lib.mi_last_error()
    assert lib.mi_pq_graph_destroy(None) == 0


def test_python_surface_raises_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd import nnsearch
    g = _NoDevice()
    for kwargs, word in [(dict(R=3), "even"), (dict(R=0), "R must"), (dict(R=66), "R must"), (dict(n_entry=0), "entry rows"),
                         (dict(n_entry=65), "entry rows")]:
        with pytest.raises(ValueError, match=word):
            _lib.PQGraphIndex.build(g, **kwargs)
    tab, ent = np.zeros((10, 4), np.int64), np.array([0, 9])
    bad = tab.copy()
    bad[3, 1] = -2
    for t, e, word in [(bad, ent, "table values"), (tab + 10, ent, "table values"), (tab, np.array([10]), "entry rows"),
                       (tab, np.array([-1]), "entry rows"), (tab[:9], ent, "table of shape"), (np.zeros((10, 65), int), ent, "table"),
                       (tab, np.zeros(65, int), "entries of shape"), (tab.astype(np.float32), ent, "integer")]:
        with pytest.raises(ValueError, match=word):
            _lib.PQGraphIndex.from_neighbors(g, t, e)
    rng = np.random.default_rng(1)
    train, test = rng.standard_normal((40, 8)).astype(np.float32), rng.standard_normal((3, 8)).astype(np.float32)
    nano = nnsearch.matching_HNSW_NanoPQ_hip
    for args, kwargs in [((0, train, test), {}), ((41, train, test), {}), ((5, train, test[:, :7]), {}), ((5, train, test), dict(m=0)),
                         ((5, train, test), dict(m=33)), ((5, train.astype(int), test), {}), ((5, train, test.astype(int)), {}),
                         ((1, train[:1], test), dict(N_words=2)), ((5, train, test), dict(N_words=8192)),
                         ((5, train, test), dict(N_words=1)), ((5, train, test), dict(N_words=64)),          # fewer rows than codewords
                         ((5, train, test), dict(N_books=3, N_words=4)), ((5, train, test), dict(N_books=65, N_words=4)),
                         ((5, train * 0, test), dict(N_words=4)), ((5, train, test * np.float32("nan")), dict(N_words=4)),
                         ((5, train[0], test), dict(N_words=4)),
                         ((1, train, test), dict(N_books=2, N_words=4, ifgenerate=False))]:
        with pytest.raises(ValueError):
            nano(*args, **kwargs)
    with pytest.raises(ValueError, match="8192"):
        nano(5, train, test, N_words=8192)
    cw = rng.standard_normal((4, 8)).astype(np.float32)              # [N_words, dim], two books of four codewords
    codes = rng.integers(0, 4, size=(40, 2))
    pq = nnsearch.matching_HNSW_PQ_hip
    for args, kwargs in [((0, cw, test, codes), {}), ((41, cw, test, codes), {}), ((5, cw, test[:, :7], codes), {}),
                         ((5, cw, test, codes), dict(m=0)), ((5, cw, test, codes), dict(m=33)), ((5, cw, test.astype(int), codes), {}),
                         ((5, cw, test * 0, codes), {}), ((5, cw, test, codes + 4), {}), ((5, cw, test, codes.astype(np.float32)), {}),
                         ((5, cw, test, codes[:, :1].repeat(3, 1)), {}), ((1, cw, test, codes[:1]), {}),
                         ((5, np.zeros((257, 8), np.float32), test, codes), {}), ((5, cw * np.float32("inf"), test, codes), {}),
                         ((5, cw[0], test, codes), {})]:
        with pytest.raises(ValueError):
            pq(*args, **kwargs)


def test_truth_is_the_brute_force_search_on_a_complete_table():
    """R = n - 1 <= 64 and ef = n: every row is reached from any entry, so the answer is the ADC top-K by (distance, id)."""
    rng = np.random.default_rng(2)
    for n, M, Ks, L in [(2, 1, 2, 3), (17, 3, 4, 2), (65, 4, 16, 1)]:
        C_ = rng.standard_normal((M, Ks, L)).astype(np.float32)
        codes = rng.integers(0, Ks, size=(n, M)).astype(np.uint8)       # (fewer codes than rows at n = 65, M = 1 .. : ties)
        q = rng.standard_normal((5, M * L)).astype(np.float32)
        table = np.array([[j for j in range(n) if j != i] for i in range(n)], np.int32)
        for k in (1, n):
            ids, dist, vis = T.search_truth(q, C_, codes, table, [n // 2], k, n, row_offset=7)
            want_ids, want_dist = P.pq_truth(q, C_, codes, k, row_offset=7)
            assert np.array_equal(ids, want_ids) and dist.tobytes() == want_dist.tobytes() and (vis == n).all()
    # a short list pads, and the table of the truth is mi_graph_build's over the ADC values of the reconstructions
    ids, dist, vis = T.search_truth(q, C_, codes, np.full((n, 1), -1, np.int32), [3, 3], 3, 8)
    assert ids[:, 0].tolist() == [3] * 5 and (ids[:, 1:] == -1).all() and np.isinf(dist[:, 1:]).all() and (vis == 1).all()
    same = np.zeros((5, 2), np.uint8)
    table, entries = T.build_truth(C_[:2], same, 2, 64)
    assert table.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]] and entries.tolist() == [0, 1, 2, 3, 4]


def test_sweep_covers_every_axis():
    cases = T.sweep_cases()
    assert len(cases) == 41 and cases[-1] == T.CEILING
    assert T.CEILING[2:4] == (64, 256) and T.CEILING[5] == 2048 and T.CEILING[0] == 3000
    for axis, want in [(0, T.NS), (3, T.KSS), (4, T.RS), (5, T.EFS), (6, T.KMODES), (7, T.NQS), (8, T.NES), (9, T.OFFS)]:
        assert {c[axis] for c in cases} == set(want), axis
    assert {(c[1], c[2]) for c in cases} == set(T.DMS)
    assert all(c[7] == 1 or c[7] * c[0] * min(c[5], c[0]) <= 3e6 for c in cases)
