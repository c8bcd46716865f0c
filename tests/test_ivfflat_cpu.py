"""CPU: the IVF-Flat index (mi_ivfflat*) is declared, exported and bound, answers bad arguments before touching a
device -- through the loaded library, through IVFFlatIndex and through matching_IVF_hip --, and its truth (tests/_ivfflat_truth.py)
does what the contract says on lists written out by hand here.
The library's checks that need the gallery's n or d (`finite`, `list ids`, `nprobe <= nlist`) cannot answer through a handle that is
never read; they are asserted on a real gallery in tests/test_gpu_ivfflat.py and, on this side, through the Python surface."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _ivfflat_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mi_ivfflat_build": 4, "mi_ivfflat_create": 6, "mi_ivfflat_info": 5, "mi_ivfflat_list_sizes": 2, "mi_ivfflat_get_lists": 3,
       "mi_ivfflat_get_centroids": 2, "mi_ivfflat_destroy": 1, "mi_ivfflat_probe_device": 6,
       "mi_ivfflat_search_device": 12}


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
    for meth in ("build", "from_lists", "train", "probe", "probe_device", "search", "search_device", "list_sizes", "lists", "centroids", "close",
                 "__enter__", "__exit__"):
        assert hasattr(_lib.IVFFlatIndex, meth), meth
    assert issubclass(_lib.IVFFlatIndex, _lib._Handle) and _lib.IVFFlatIndex.close is _lib._Handle.close
    assert _lib.IVFFlatIndex._DESTROY == "mi_ivfflat_destroy"
    assert list(inspect.signature(_lib.IVFFlatIndex.build).parameters) == ["gallery", "centroids"]
    assert list(inspect.signature(_lib.IVFFlatIndex.from_lists).parameters) == ["gallery", "centroids", "list_ids"]
    p = inspect.signature(_lib.IVFFlatIndex.search).parameters
    assert list(p)[:6] == ["self", "q", "k", "nprobe", "probes", "allow"]
    assert p["nprobe"].default == 1 and p["probes"].default is None and p["allow"].default is None
    assert inspect.signature(_lib.IVFFlatIndex.probe).parameters["nprobe"].default == 1
    p = inspect.signature(_lib.IVFFlatIndex.train).parameters
    assert list(p) == ["x", "nlist", "iters", "seed", "device"]
    assert p["iters"].default == 20 and p["seed"].default == 0 and p["device"].default == 0
    assert _lib.IVFFLAT_SLAB_ROWS == 2048
    kernels = open(os.path.join(ROOT, "image-search-engine-for-historical-research_amd", "csrc", "kernels.h")).read()
    assert "IVFFLAT_SLAB_ROWS = %d;" % _lib.IVFFLAT_SLAB_ROWS in kernels
    from isehr_amd import build
    for src in ("api_ivfflat.hip", "ivfflat.hip"):
        assert src in build.SOURCES
        assert os.path.exists(os.path.join(build.CSRC, src))


def test_matcher_is_registered():
    from isehr_amd import nnsearch
    assert nnsearch.MATCHING_METHODS["IVF"] is nnsearch.matching_IVF_hip
    p = inspect.signature(nnsearch.matching_IVF_hip).parameters
    assert list(p) == ["K", "embedded_features_train", "embedded_features_test", "dataset", "nlist", "nprobe", "metric", "ifgenerate"]
    assert p["dataset"].default is None and p["nlist"].default is None and p["nprobe"].default == 8
    assert p["metric"].default == "euclidean" and p["ifgenerate"].default is True
    assert nnsearch.ivfflat_default_nlist(0) == 2 and nnsearch.ivfflat_default_nlist(1) == 4 and nnsearch.ivfflat_default_nlist(2000) == 179
    assert nnsearch.ivfflat_default_nlist(1005994) == 4012 and nnsearch.ivfflat_default_nlist(10 ** 7) == 8192


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    idx = np.zeros(16, np.int64)
    cent = np.zeros((2, 4), np.float32)
    lids = np.zeros(10, np.int32)
    out = C.c_void_p()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def dev(f=fake, qp=P(q), nq=2, k=4, nprobe=1, op=P(idx)):
        return lib.mi_ivfflat_search_device(f, qp, nq, k, nprobe, None, None, op, None, None, None, None)

    for call in (dev,):
        for kwargs, word in [(dict(f=None), b"null handle"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"), (dict(nq=-1), b"nq"),
                             (dict(nprobe=0), b"nprobe"), (dict(nprobe=8193), b"nprobe"), (dict(qp=None), b"queries"),
                             (dict(op=None), b"out_idx")]:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
        assert call(nq=0, qp=None, op=None) == 0                  # nq == 0: MI_OK, nothing read, nothing written

    def probe(f=fake, qp=P(q), nq=2, nprobe=1, op=P(idx)):
        return lib.mi_ivfflat_probe_device(f, qp, nq, nprobe, op, None)

    for kwargs, word in [(dict(f=None), b"null handle"), (dict(nq=-1), b"nq"), (dict(nprobe=0), b"nprobe"), (dict(qp=None), b"queries"),
                         (dict(nprobe=8193), b"nprobe"), (dict(op=None), b"out_probes")]:
        assert probe(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert probe(nq=0, qp=None, op=None) == 0
    assert (idx == 0).all()

    def build(g=fake, cp=P(cent), nlist=2, o=C.byref(out)):
        return lib.mi_ivfflat_build(g, cp, nlist, o)

    def create(g=fake, cp=P(cent), nlist=2, lp=P(lids), space=0, o=C.byref(out)):
        return lib.mi_ivfflat_create(g, cp, nlist, lp, space, o)

    common = [(dict(g=None), b"null handle"), (dict(cp=None), b"centroids"), (dict(o=None), b"out"), (dict(nlist=1), b"nlist must"),
              (dict(nlist=8193), b"nlist must")]
    for call, cases in [(build, common), (create, common + [(dict(lp=None), b"list_ids"), (dict(space=7), b"memspace")])]:
        for kwargs, word in cases:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
    assert out.value is None
    assert lib.mi_ivfflat_info(None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfflat_list_sizes(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfflat_get_lists(None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfflat_get_centroids(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfflat_destroy(None) == 0


def test_python_surface_raises_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd import nnsearch
    g = _NoDevice()                                           # n = 10, d = 4
    cent = np.zeros((3, 4), np.float32)
    nan = cent.copy()
    nan[1, 2] = np.nan
    for c, word in [(cent[:1], "nlist = 1"), (np.zeros((8193, 4), np.float32), "nlist = 8193"), (np.zeros((3, 5), np.float32), "columns"),
                    (nan, "finite"), (np.zeros(4, np.float32), "\\[nlist, d\\]"), (np.zeros((3, 4), bool), "numeric")]:
        with pytest.raises(ValueError, match=word):
            _lib.IVFFlatIndex.build(g, c)
        with pytest.raises(ValueError, match=word):
            _lib.IVFFlatIndex.from_lists(g, c, np.zeros(10, np.int32))
    for li, word in [(np.zeros(9, np.int32), "list ids must be \\[n = 10\\]"), (np.zeros(10, np.float32), "integer"),
                     (np.full(10, 3), "lie in"), (np.full(10, -1), "lie in"), (np.zeros((10, 1), np.int32), "list ids must be")]:
        with pytest.raises(ValueError, match=word):
            _lib.IVFFlatIndex.from_lists(g, cent, li)
    empty = _NoDevice()
    empty.n = 0
    with pytest.raises(ValueError, match="rows"):
        _lib.IVFFlatIndex.build(empty, cent)
    for nlist in (1, 8193):
        with pytest.raises(ValueError, match="nlist = %d" % nlist):
            _lib.IVFFlatIndex.train(np.zeros((10, 4), np.float32), nlist)
    assert _lib.ivfflat_centroids(np.zeros((1, 3, 4)), 4).shape == (3, 4)       # what pq_train(x, 1, nlist) returns
    train, test = np.zeros((20, 4), np.float32), np.zeros((3, 4), np.float32)
    for args, kwargs in [((0, train, test), {}), ((21, train, test), {}), ((5, train, test[:, :3]), {}), ((5, train, test), dict(nlist=1)),
                         ((5, train, test), dict(nlist=21)), ((5, train, test), dict(nlist=4, nprobe=5)),
                         ((5, train, test), dict(nlist=4, nprobe=0)), ((5, train.astype(int), test), {}),
                         ((5, train, test), dict(metric="manhattan")), ((1, train, test), dict(ifgenerate=False)),
                         ((5, train, test), dict(metric="angular")), ((2049, np.zeros((3000, 4), np.float32), test), {})]:
        with pytest.raises(ValueError):
            nnsearch.matching_IVF_hip(*args, **kwargs)


def test_truth_on_lists_written_out_by_hand():
    """Six rows on a line, three centroids at 0, 10 and 20 (the last one owns nothing)."""
    rows = np.array([[0.0], [9.0], [1.0], [11.0], [5.0], [10.0]], np.float32)
    cent = np.array([[0.0], [10.0], [20.0]], np.float32)
    lid = T.assign(rows, cent, True)
    assert lid.tolist() == [0, 1, 0, 1, 0, 1] and lid.dtype == np.int32          # row 4 ties at 25: the lower list
    off, lr = T.lists_of(lid, 3)
    assert off.tolist() == [0, 3, 6, 6] and lr.tolist() == [0, 2, 4, 1, 3, 5] and off.dtype == np.int64 and lr.dtype == np.int32
    assert T.probe(np.array([[5.0], [16.0]], np.float32), cent, 2, True).tolist() == [[0, 1], [2, 1]]
    assert T.probe(np.array([[1.0], [-1.0]], np.float32), cent, 3, False).tolist() == [[2, 1, 0], [0, 1, 2]]
    assert T.normalise([[1, 1, 3, -1, 0, 1], [2, 2, 2, 0, 0, -7]], 3).tolist() == [[1, -1, -1, -1, 0, -1], [2, -1, -1, 0, -1, -1]]
    q = np.array([[10.0]], np.float32)
    ids, vals, scanned = T.search(q, rows, [[1, 2]], off, lr, 3, 4, True, row_offset=100)
    assert ids.tolist() == [[105, 101, 103, -1]] and vals.tolist() == [[0.0, 1.0, 1.0, np.inf]] and scanned.tolist() == [3]
    allow = np.array([1, 0, 1, 1, 1, 1], bool)
    ids, vals, scanned = T.search(q, rows, [[1, 0, 1]], off, lr, 3, 3, True, allow=allow)
    assert ids.tolist() == [[5, 3, 4]] and vals.tolist() == [[0.0, 1.0, 25.0]] and scanned.tolist() == [5]
    ids, vals, scanned = T.search(q, rows, [[2, -1]], off, lr, 3, 2, False)
    assert ids.tolist() == [[-1, -1]] and vals.tolist() == [[-np.inf, -np.inf]] and scanned.tolist() == [0]
    ids, vals, _ = T.search(np.array([[1.0]], np.float32), rows, [[0, 1]], off, lr, 3, 2, False)
    assert ids.tolist() == [[3, 5]] and vals.tolist() == [[11.0, 10.0]]
    assert T.lattice(np.random.default_rng(0), (50, 3)).dtype == np.float32
    assert set(np.unique(T.lattice(np.random.default_rng(0), (500, 3)))) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
