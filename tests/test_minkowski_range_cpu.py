"""CPU: the Minkowski radius search (mi_range_search_minkowski, mi_range_search_minkowski_device, mi_minkowski_self_range; DESIGN.md
5.19b) as far as no device is needed: the refusals of the binding before the library loads, the routing of KNN.radius_search, the
refusals of the library before a handle is read, the global option, and the numpy truth tests/test_gpu_minkowski_range.py uses."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _minkowski_range_truth as R
import _minkowski_truth as T

NEW = ["mi_range_search_minkowski", "mi_range_search_minkowski_device", "mi_minkowski_self_range"]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_binding_refuses_before_the_library_loads():
    from isehr_amd import _lib
    assert _lib.minkowski_range_args("l1", None, 0) == (_lib.MINK_L1, 0.0, 0.0)
    assert _lib.minkowski_range_args("linf", 3.0, math.inf) == (_lib.MINK_LINF, 0.0, math.inf)
    assert _lib.minkowski_range_args("lp", 2, 1.5) == (_lib.MINK_LP, 2.0, 1.5)
    for metric, p, radius in (("l2", None, 1.0), ("lp", 0.0, 1.0), ("lp", -1.0, 1.0), ("lp", None, 1.0), ("lp", math.nan, 1.0),
                              ("l1", None, math.nan), ("l1", None, -1e-300), ("linf", None, -math.inf)):
        with pytest.raises(ValueError):
            _lib.minkowski_range_args(metric, p, radius)
    # the entry points of the binding run those checks first: there is no handle and no library is loaded
    g = _lib.Gallery.__new__(_lib.Gallery)
    g._h, g.d = None, 4
    q = np.zeros((2, 4), np.float32)
    for kw in (dict(metric="cityblock"), dict(metric="lp", p=0), dict(metric="lp", p=math.inf), dict(radius=math.nan),
               dict(radius=-0.5)):
        args = dict(radius=1.0, metric="l1", p=None)
        args.update(kw)
        with pytest.raises(ValueError):
            g.range_search_minkowski(q, **args)
        with pytest.raises(ValueError):
            g.range_search_minkowski_device(0, 2, args["radius"], 0, 0, 0, metric=args["metric"], p=args["p"])
        with pytest.raises(ValueError):
            g.self_range_minkowski(0, 2, args["radius"], args["metric"], args["p"])
    with pytest.raises(ValueError, match="dimension"):
        g.range_search_minkowski(np.zeros((2, 5), np.float32), 1.0)             # another width than the gallery's


def test_knn_radius_search_routing():
    from isehr_amd.knn import KNN
    calls = []

    class FakeGallery:
        def range_search_minkowski(self, q, radius, metric="l1", p=None, allow=None, max_results=None):
            calls.append((q.dtype, q.shape, radius, metric, p))
            lims = np.arange(q.shape[0] + 1, dtype=np.int64)
            return (lims, np.arange(q.shape[0], dtype=np.int64), np.ones(q.shape[0], np.float32), np.ones(q.shape[0], np.float64), 0.0)

    def knn_of(method, p=None):
        knn = object.__new__(KNN)
        knn.gallery, knn.method, knn.p, knn.N, knn.D = FakeGallery(), method, p, 10, 4
        return knn

    q64 = np.zeros((3, 4), np.float64)
    for method, p, want in (("euclidean", None, ("lp", 2.0)), ("l1", None, ("l1", None)), ("linf", None, ("linf", None)),
                            ("lp", 0.5, ("lp", 0.5))):
        del calls[:]
        lims, dist, ids = knn_of(method, p).radius_search(q64, 2)
        assert calls == [(np.float32, (3, 4), 2.0) + want]
        assert lims.dtype == np.int64 and dist.dtype == np.float32 and ids.dtype == np.int64 and lims.tolist() == [0, 1, 2, 3]
        with pytest.raises(NotImplementedError):                               # range_search stays what it was
            knn_of(method, p).range_search(q64, 0.5)
        for bad in (math.nan, -1.0):
            with pytest.raises(ValueError):
                knn_of(method, p).radius_search(q64, bad)
    for method in ("cosine", "hamming"):
        with pytest.raises(NotImplementedError, match="range_search"):
            knn_of(method).radius_search(q64, 1.0)
    assert len(calls) == 1


def test_symbols_header_and_option(built_lib):
    lib, _lib = built_lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and getattr(lib, name).restype == C.c_int, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [17, 13, 12]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mi355_retrieval.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
    cap = re.search(r"MI_ERR_CAPACITY = 7\s*/\*(.*?)\*/", hdr, re.S).group(1)
    assert all(name in cap for name in NEW)
    assert "\"minkowski_range_bytes\"" in hdr
    assert _lib.get_global_option("minkowski_range_bytes") == 256 << 20
    try:
        _lib.set_global_option("minkowski_range_bytes", 4096)
        assert _lib.get_global_option("minkowski_range_bytes") == 4096
    finally:
        _lib.set_global_option("minkowski_range_bytes", 0)
    assert _lib.get_global_option("minkowski_range_bytes") == 256 << 20
    assert lib.mi_set_global_option(b"minkowski_range_bytes", -1.0) == _lib.MI_ERR_INVALID
    assert b"minkowski_range_bytes" in lib.mi_last_error()


def test_library_refuses_before_the_handle_is_read(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    lims, idx = np.full(3, -5, np.int64), np.zeros(8, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def host(g=fake, nq=2, dtype=_lib.MI_F32, metric=_lib.MINK_L1, p=0.0, radius=1.0, cap=8, lims_p=P(lims), idx_p=P(idx), space=0):
        return lib.mi_range_search_minkowski(g, P(q), nq, dtype, 4, 1, metric, p, radius, None, space, cap, lims_p, idx_p, None, None, None)

    for kw, word in [(dict(g=None), b"null"), (dict(metric=0), b"metric"), (dict(metric=4), b"metric"),
                     (dict(metric=_lib.MINK_LP, p=0.0), b"p must"), (dict(metric=_lib.MINK_LP, p=math.nan), b"p must"),
                     (dict(radius=math.nan), b"radius"), (dict(radius=-1.0), b"radius"), (dict(nq=-1), b"nq"),
                     (dict(lims_p=None), b"out_lims"), (dict(cap=-1), b"max_results"), (dict(idx_p=None), b"out_idx"),
                     (dict(dtype=9), b"dtype")]:
        assert host(**kw) == _lib.MI_ERR_INVALID, kw
        assert word in lib.mi_last_error(), (kw, lib.mi_last_error())
    assert (lims == -5).all()
    assert host(nq=0) == 0 and lims.tolist() == [0, -5, -5]                     # nq == 0: MI_OK, lims[0] written
    assert host(nq=0, cap=0, idx_p=None, radius=math.inf) == 0
    dev = lambda **kw: lib.mi_range_search_minkowski_device(  # noqa: E731
        kw.get("g", fake), P(q), kw.get("nq", 2), kw.get("metric", 1), 0.0, kw.get("radius", 1.0), None, kw.get("cap", 8),
        kw.get("lims_p", P(lims)), kw.get("idx_p", P(idx)), None, None, None)
    for kw in (dict(g=None), dict(metric=7), dict(radius=-2.0), dict(radius=math.nan), dict(nq=-1), dict(lims_p=None), dict(cap=-1),
               dict(idx_p=None)):
        assert dev(**kw) == _lib.MI_ERR_INVALID, kw
    own = lambda **kw: lib.mi_minkowski_self_range(  # noqa: E731
        kw.get("g", fake), kw.get("row0", 0), kw.get("nrows", 1), kw.get("metric", 1), 0.0, kw.get("radius", 1.0), kw.get("cap", 8),
        kw.get("lims_p", P(lims)), kw.get("idx_p", P(idx)), None, None, None)
    for kw in (dict(g=None), dict(metric=0), dict(radius=-2.0), dict(radius=math.nan), dict(row0=-1), dict(nrows=-1), dict(lims_p=None),
               dict(cap=-1), dict(idx_p=None)):
        assert own(**kw) == _lib.MI_ERR_INVALID, kw


def test_truth_csr_contract():
    vals = np.array([[3.0, 1.0, math.nan, 1.0, 0.0, math.inf],
                     [9.0, 9.0, 9.0, 9.0, 9.0, 9.0],
                     [0.0, 0.0, 5.0, 0.0, 2.0, 1.0]])
    lims, ids, dist = R.csr(vals, 2.0, row_offset=10)
    assert lims.tolist() == [0, 3, 3, 8] and ids.tolist() == [14, 11, 13, 10, 11, 13, 15, 14]
    assert dist.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 2.0]
    assert R.csr(vals, 1.0)[0].tolist() == [0, 3, 3, 7]                        # inclusive
    assert R.csr(vals, np.nextafter(1.0, -np.inf))[0].tolist() == [0, 1, 1, 4]
    lims, ids, _ = R.csr(vals, math.inf)
    assert lims.tolist() == [0, 5, 11, 17] and 2 not in ids[:5].tolist()       # +inf: everything but the NaN
    lims, ids, _ = R.csr(vals, 2.0, allow=np.arange(6) % 3 == 0)
    assert lims.tolist() == [0, 1, 1, 3] and ids.tolist() == [3, 0, 3]
    lims, ids, _ = R.csr(vals, 2.0, above=[3, 0, 1])                           # the self-join keeps the rows above the query's
    assert lims.tolist() == [0, 1, 1, 4] and ids.tolist() == [4, 3, 5, 4]
    assert R.csr(vals, 2.0, allow=np.zeros(6, bool))[0].tolist() == [0, 0, 0, 0]
    assert R.csr(np.zeros((0, 4)), 1.0)[0].tolist() == [0]


def test_truth_pairs_and_values():
    rng = np.random.default_rng(3)
    rows = rng.integers(-2, 3, (40, 6)).astype(np.float32)
    rows[31] = rows[7]
    vals = R.values(rows, rows, "l1")
    assert np.array_equal(vals, T.values(rows, rows, "l1")) and (np.diag(vals) == 0).all()
    pr, dist = R.pairs(vals, 3.0)
    want = [(i, j) for i in range(40) for j in range(i + 1, 40) if vals[i, j] <= 3.0]
    assert sorted(map(tuple, pr.tolist())) == want and (pr[:, 0] < pr[:, 1]).all() and len(set(map(tuple, pr.tolist()))) == len(pr)
    assert [7, 31] in pr.tolist() and np.array_equal(dist, vals[pr[:, 0], pr[:, 1]])
    for i in np.unique(pr[:, 0]):                                              # per i: (value asc, j asc)
        seg = pr[:, 0] == i
        assert np.array_equal(np.lexsort((pr[seg, 1], dist[seg])), np.arange(seg.sum()))


def test_chunk_plan_under_sanitizers(tmp_path):
    """csrc/mink_range_plan.h (queries per chunk within "minkowski_range_bytes") over a sweep of shapes: tests/mink_range_plan_check.cpp,
    compiled with the host compiler under AddressSanitizer and UBSan and run as a program of its own; nothing is loaded into Python."""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "mink_range_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", os.path.join(here, "mink_range_plan_check.cpp"), "-o", exe]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + sanitize + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base + sanitize, capture_output=True, text=True)
    if r.returncode != 0:                          # the sanitizer runtimes are a package of their own: the program's checks still run
        assert "sanitizer" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr[-3000:]
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0 and "mink_range_plan_check ok" in run.stdout
